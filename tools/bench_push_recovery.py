"""kbj_push_recovery alone, at the sweep's default shape and at the workload's shape, with and without the group statistics, against its
traffic floor.

usage: python tools/bench_push_recovery.py [--reps 20] [--warmup 5]

Shapes: the default task.push_sweep() (T = 260 rows: push at row 100 for 10 rows, window 150, hold 25; N = 128 envs in G = 32 cases) and
T = 100, N = 8192 (push rows drawn in [25, 40), 10 rows, window 50, hold 25; G = 32). Synthetic rows: errors within the tolerances but for a
tenth of the rows, an episode end every ~300 steps. Kernel time: HIP events around the ABI call (the scan, and with stats_d the
single-workgroup second stage), `warmup` untimed calls, then the median of `reps`. Floor: the bytes a call needs - for every env the err_d
rows [s - hold, min(T, s + d + window)) at 32 bytes and their DONE words at 4, the schedule and the result row - over the rate this
project has measured for a streaming kernel of its own (tools/bench_tracking_stats.py: 4.02 TB/s). The DONE words sit 288 bytes apart in
the aux rows, so the hardware moves more than the floor counts. Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stats_bench import STREAM_TBPS, floor_us, timed_call      # noqa: E402 (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.spec import compiler, layout as L
    dev = torch.device("cuda", 0)
    ctx = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=64, batch_size=64, hidden_size=64, rollout_len=8))
    X, R = L.AUX, L.TERR
    out = dict(stream_tb_per_s=round(STREAM_TBPS, 2))
    for name, T, N, G, s_lo, s_hi, d, window, hold in (("sweep_default", 260, 128, 32, 100, 101, 10, 150, 25), ("workload", 100, 8192, 32, 25, 40, 10, 50, 25)):
        g = torch.Generator(device=dev); g.manual_seed(0)
        err = torch.rand(T, N, R["SIZE"], device=dev, generator=g) * 0.9
        err[:, :, 0] += (torch.rand(T, N, device=dev, generator=g) < 0.1).float()                      # a tenth of the rows leave the tolerance of 1
        aux = torch.zeros(T + 1, N, X["SIZE"], device=dev)
        u = torch.rand(T, N, device=dev, generator=g)
        aux[:T, :, X["DONE"]] = torch.where(u < 1 / 600, -1.0, torch.where(u < 1 / 300, 1.0, 0.0))
        sched = torch.stack([torch.randint(s_lo, s_hi, (N,), device=dev, generator=g), torch.full((N,), d, device=dev)], 1).to(torch.int32).contiguous()
        group = (torch.arange(N, device=dev) % G).to(torch.int32)
        rec = torch.zeros(N, L.PREC["SIZE"], device=dev)
        stats = torch.zeros(G, L.PSTAT["SIZE"], dtype=torch.float64, device=dev)
        crit = B.PushCriteria((B.C.c_float * L.NTERR)(1.0, 1.0, 1.0, float("inf"), 1.0), hold, window)
        traj = B.Traj(T=T, N=N, aux_d=aux.data_ptr())
        s = sched[:, 0].cpu().numpy()
        rows = int(sum(min(T, x + d + window) - (x - hold) for x in s))
        nbytes = rows * (R["SIZE"] * 4 + 4) + N * (8 + L.PREC["SIZE"] * 4)
        res = dict(T=T, N=N, G=G, needed_mb=round(nbytes / 1e6, 3), floor_us=round(floor_us(nbytes), 3))
        for leg, st in (("rec_only", None), ("with_stats", stats)):
            us, res[leg] = timed_call(lambda: ctx.push_recovery(traj, err, sched, crit, rec, group, G, st), a.reps, a.warmup)
            res[leg]["ratio_to_floor"] = round(us / res["floor_us"], 1)
        res["outcomes"] = [int(x) for x in stats.cpu().numpy()[:, :L.POUT["COUNT"]].sum(0)]
        out[name] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
