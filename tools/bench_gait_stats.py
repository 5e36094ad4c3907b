"""kbj_gait_stats alone at the workload's shape, with and without the per-env record, beside kbj_tracking_stats on the same aux rows in the same
run, against their common traffic floor; with --scalars, what scalars() costs a training task with the gait switch on.

usage: python tools/bench_gait_stats.py [--envs 8192] [--steps 100] [--reps 20] [--warmup 5] [--scalars]

Kernel time: HIP events around the ABI call (both launches: the scan and the single-workgroup reduce), `warmup` untimed calls, then the
median of `reps`. Floor: every aux row [T][N][72] fp32 read once (236 MB at 100 x 8192; the gait kernel skips 5 of the 18 16-byte pieces of a
row, but whole 128-byte lines travel, so the floor keeps them) over the rate this project has measured for a streaming kernel of its own:
adamw_kernel moves 63.05 MB per launch (profiles/pmc_traffic.json) in 15.7 us (profiles/r06zz_rocprofv3_kernel_stats.md) = 4.02 TB/s.
--scalars: a task of `envs` x `steps` at hidden size 64 with gait_stats on and off, the median wall time of scalars() behind a synchronised
iteration. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stats_bench import STREAM_TBPS, floor_us, timed_call      # noqa: E402 (tools/ is the script's directory)


def _scalars_cost(envs, steps, reps):
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
    out = {}
    for name, on in (("gait_off", False), ("gait_on", True)):
        cfg = launch_config(num_envs=envs, batch_size=min(envs, 512), hidden_size=64, num_passes=1, rollout_length_seconds=steps * 0.02, robot="kbot-headless", gait_stats=on)
        task = HumanoidWalkingTask(cfg)
        ms = []
        for _ in range(reps):
            task.train_iteration()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc = task.scalars()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(scalars_ms_median=round(statistics.median(ms), 3), scalars_ms_min=round(min(ms), 3), keys=len(sc))
        task.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scalars", action="store_true")
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
    # a walking contact pattern: each foot down 15 rows of every 25, the right half a period late, every env at its own phase
    t = torch.arange(T, device=dev)[:, None] + torch.randint(0, 25, (N,), device=dev, generator=g)[None, :]
    down = torch.stack([(t % 25) < 15, ((t + 12) % 25) < 15], dim=-1)
    aux[:T, :, X["TOUCH"]:X["TOUCH"] + 2] = torch.where(down, 200.0 + 100.0 * aux[:T, :, X["TOUCH"]:X["TOUCH"] + 2], 0.0)
    aux[:T, :, X["LFZ"]], aux[:T, :, X["RFZ"]] = torch.where(down[..., 0], 0.04, 0.04 + 0.05 * aux[:T, :, X["LFZ"]].abs()), torch.where(down[..., 1], 0.04, 0.04 + 0.05 * aux[:T, :, X["RFZ"]].abs())
    aux[:T, :, X["CTRL"]:X["CTRL"] + L.NU] *= 30.0
    traj = B.Traj(T=T, N=N, aux_d=aux.data_ptr())                                     # the aux rows are all either kernel reads
    nbytes = T * N * X["SIZE"] * 4
    floor = floor_us(nbytes)
    out = dict(envs=N, steps=T, stream_tb_per_s=round(STREAM_TBPS, 2), moved_mb=round(nbytes / 1e6, 2), floor_us=round(floor, 2))
    gacc, gstats, genv = torch.zeros(N, L.GACC["SIZE"], device=dev), torch.zeros(L.GAIT["SIZE"], dtype=torch.float64, device=dev), torch.zeros(N, L.GENV["SIZE"], device=dev)
    tacc, tstats = torch.zeros(N, L.TACC["SIZE"], device=dev), torch.zeros(L.TRK["SIZE"], dtype=torch.float64, device=dev)
    calls = (("gait_stats_only", lambda: ctx.gait_stats(traj, gacc, gstats)), ("gait_with_env", lambda: ctx.gait_stats(traj, gacc, gstats, genv)),
             ("tracking_stats_only", lambda: ctx.tracking_stats(traj, 25, tacc, tstats)))
    for name, call in calls:
        us, out[name] = timed_call(call, a.reps, a.warmup, "kernel_")
        out[name]["ratio_to_floor"] = round(us / floor, 2)
    v = gstats.cpu().numpy()
    out["rows_per_mode"] = [float(v[L.gait_slot(m, "ROWS")]) for m in range(L.CMODE["COUNT"])]
    out["touchdowns"] = float(sum(v[L.gait_slot(m, "TOUCHDOWNS", f)] for m in range(L.CMODE["COUNT"]) for f in range(2)))
    out["counted_swings"] = float(sum(v[L.gait_slot(m, "SWING_N", f)] for m in range(L.CMODE["COUNT"]) for f in range(2)))
    ctx.close()
    if a.scalars:
        out["scalars"] = _scalars_cost(N, T, max(3, a.reps // 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
