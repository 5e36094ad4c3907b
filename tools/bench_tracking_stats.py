"""kbj_tracking_stats alone at the workload's shape, with and without the per-row output, against its traffic floor.

usage: python tools/bench_tracking_stats.py [--envs 8192] [--steps 100] [--settle 25] [--reps 20] [--warmup 5]

Kernel time: HIP events around the ABI call (both launches: the scan and the single-workgroup reduce), `warmup` untimed calls, then the
median of `reps`. Floor: the bytes the kernel moves - every aux row [T][N][72] fp32 read once (236 MB at 100 x 8192) and, with err_d, the
rows [T][N][8] fp32 written (26 MB) - over the rate this project has measured for a streaming kernel of its own: adamw_kernel moves
63.05 MB per launch (profiles/pmc_traffic.json) in 15.7 us (profiles/r06zz_rocprofv3_kernel_stats.md) = 4.02 TB/s. Prints one JSON line."""
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--settle", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.spec import compiler, layout as L
    dev = torch.device("cuda", 0)
    T, N = a.steps, a.envs
    ctx = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=N, batch_size=min(N, 512), rollout_len=T))
    g = torch.Generator(device=dev); g.manual_seed(0)
    X = L.AUX
    aux = torch.rand(T + 1, N, X["SIZE"], device=dev, generator=g) * 2 - 1
    aux[:, :, X["BQUAT"]] += 2.0                                                      # a base near upright
    cmd = torch.zeros(T, N, L.NCMD, device=dev)
    modes = torch.randint(0, 6, (N,), device=dev, generator=g)                      # one command per env and call, a sixth of the envs per mode
    cmd[:, modes == 0, 0], cmd[:, modes == 1, 1], cmd[:, modes == 2, 2] = 0.7, 0.3, 0.5
    cmd[:, modes == 3, :3], cmd[:, modes == 3, 6] = 0.4, 0.3
    cmd[:, modes == 4, 3] = -0.1
    cmd[T // 2:, : N // 4, 0] += 0.1                                                  # a quarter of the envs switch mid-way
    aux[:T, :, X["CMD"]:X["CMD"] + L.NCMD] = cmd
    u = torch.rand(T, N, device=dev, generator=g)
    aux[:T, :, X["DONE"]] = torch.where(u < 1 / 300, -1.0, torch.where(u < 1 / 150, 1.0, 0.0))     # an episode ends every ~150 steps
    traj = B.Traj(T=T, N=N, aux_d=aux.data_ptr())                                     # the aux rows are all the kernel reads
    acc = torch.zeros(N, L.TACC["SIZE"], device=dev)
    stats = torch.zeros(L.TRK["SIZE"], dtype=torch.float64, device=dev)
    err = torch.zeros(T, N, L.TERR["SIZE"], device=dev)
    out = dict(envs=N, steps=T, settle_steps=a.settle, stream_tb_per_s=round(STREAM_TBPS, 2))
    for name, e in (("stats_only", None), ("with_err", err)):
        us, out[name] = timed_call(lambda: ctx.tracking_stats(traj, a.settle, acc, stats, e), a.reps, a.warmup, "kernel_")
        nbytes = T * N * X["SIZE"] * 4 + (0 if e is None else T * N * L.TERR["SIZE"] * 4)
        out[name].update(moved_mb=round(nbytes / 1e6, 2), floor_us=round(floor_us(nbytes), 2), ratio=round(us / floor_us(nbytes), 2))
    v = stats.cpu().numpy()
    S = L.TRK["MODE_STRIDE"]
    out["rows_per_mode"] = [float(v[m * S + L.TRK["ROWS"]]) for m in range(L.CMODE["COUNT"])]
    out["settled_per_mode"] = [float(v[m * S + L.TRK["SETTLED"]]) for m in range(L.CMODE["COUNT"])]
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
