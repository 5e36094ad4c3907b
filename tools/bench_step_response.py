"""kbj_step_response alone at the default sweep's length and a wide env count, with and without the group statistics, against its traffic floor.

usage: python tools/bench_step_response.py [--envs 8192] [--steps 350] [--reps 20] [--warmup 5]

Shape: T = 350 rows, the step on row 150, window 200, hold 25, smoothing over 25 rows (task.step_sweep()'s defaults at ctrl_dt = 0.02 s), N envs in
G = 10 cases. Synthetic aux rows: a first-order response of the forward velocity (time constant 15 rows) with a little noise under random
attitudes, an episode end every ~2000 steps, so that most envs settle some 40 rows behind the step and the scan stops early, as a policy that
follows its stick would make it. A second leg (`never_settles`) holds the velocity at the old command: every env scans its whole window.
Kernel time: HIP events around the ABI call (the signal kernel, the scan and, with stats_d, the single-workgroup second stage), `warmup`
untimed calls, then the median of `reps`. Floor: the bytes a call needs - for every row the 14 aux words stage 1 reads and the 32 bytes it
writes, for every env the signal rows [s - hold, deciding row] re-read at 32 bytes, the schedule and the record - over the rate this project
has measured for a streaming kernel of its own (tools/bench_tracking_stats.py: 4.02 TB/s). The aux words of a row lie in three places of its
288 bytes, so the hardware moves more than the floor counts. Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stats_bench import STREAM_TBPS, floor_us, timed_call      # noqa: E402 (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=350)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.spec import compiler, layout as L
    dev = torch.device("cuda", 0)
    ctx = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=64, batch_size=64, hidden_size=64, rollout_len=8))
    X, R, S, O = L.AUX, L.SREC, L.SSTAT, L.SOUT
    T, N, G = a.steps, a.envs, 10
    s, window, hold, m = 150 * T // 350, 200 * T // 350, 25, 25
    out = dict(stream_tb_per_s=round(STREAM_TBPS, 2), T=T, N=N, G=G, step_row=s, window=window, hold=hold, smooth=m)
    f3 = B.C.c_float * L.NSCH
    crit = B.StepCriteria(f3(0.05, 0.05, 0.05), f3(0.15, 0.15, 0.25), 0.1, 0.9, m, hold, window)
    sched = torch.full((N,), s, dtype=torch.int32, device=dev)
    group = (torch.arange(N, device=dev) % G).to(torch.int32)
    sig = torch.zeros(T, N, L.SSIG["SIZE"], device=dev)
    rec = torch.zeros(N, R["SIZE"], device=dev)
    stats = torch.zeros(G, S["SIZE"], dtype=torch.float64, device=dev)
    for name, tau in (("settles", 15.0), ("never_settles", None)):
        g = torch.Generator(device=dev); g.manual_seed(0)
        aux = torch.rand(T + 1, N, X["SIZE"], device=dev, generator=g) - 0.5
        yaw = torch.rand(T + 1, N, device=dev, generator=g) * 6.2831853
        aux[:, :, X["BQUAT"]], aux[:, :, X["BQUAT"] + 3] = torch.cos(0.5 * yaw), torch.sin(0.5 * yaw)
        aux[:, :, X["BQUAT"] + 1:X["BQUAT"] + 3] *= 0.05
        k = (torch.arange(T + 1, device=dev, dtype=torch.float32) - s + 1).clamp(min=0)[:, None]
        v = (1.0 - torch.exp(-k / tau) if tau else torch.zeros_like(k)) * (k > 0) + 0.02 * (torch.rand(T + 1, N, device=dev, generator=g) - 0.5)
        aux[:, :, X["QVEL"]], aux[:, :, X["QVEL"] + 1] = torch.cos(yaw) * v, torch.sin(yaw) * v      # forward speed v in the heading frame
        aux[:, :, X["QVEL"] + 5] = 0.02 * (torch.rand(T + 1, N, device=dev, generator=g) - 0.5)
        aux[:, :, X["CMD"]:X["CMD"] + L.NCMD] = 0.0
        aux[s:, :, X["CMD"]] = 1.0
        u = torch.rand(T + 1, N, device=dev, generator=g)
        aux[:, :, X["DONE"]] = torch.where(u < 1 / 4000, -1.0, torch.where(u < 1 / 2000, 1.0, 0.0))
        traj = B.Traj(T=T, N=N, aux_d=aux.data_ptr())
        res = {}
        for leg, st in (("rec_only", None), ("with_stats", stats)):
            res[leg] = timed_call(lambda: ctx.step_response(traj, sched, crit, sig, rec, group, G, st), a.reps, a.warmup)[1]
        r = rec.cpu().numpy()
        oc = r[:, R["OUTCOME"]].astype(int)
        # the rows an env's lane re-reads: the hold rows in front, then up to its deciding row (VOID on a row in front: counted in full, an upper bound)
        scanned = [hold + (int(x[R["SETTLE_STEPS"]]) + hold if o == O["SETTLED"] else int(x[R["FALL_STEPS"]]) + 1 if o == O["FELL"] else min(window, T - s)) if o != O["NONE"] else 0
                   for x, o in zip(r, oc)]
        nbytes = T * N * (14 * 4 + L.SSIG["SIZE"] * 4) + sum(scanned) * L.SSIG["SIZE"] * 4 + N * (4 + R["SIZE"] * 4)
        res.update(needed_mb=round(nbytes / 1e6, 3), floor_us=round(floor_us(nbytes), 3), outcomes=[int((oc == i).sum()) for i in range(O["COUNT"])])
        for leg in ("rec_only", "with_stats"):
            res[leg]["ratio_to_floor"] = round(res[leg]["us_median"] / res["floor_us"], 1)
        out[name] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
