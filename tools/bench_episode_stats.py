"""kbj_episode_stats alone at the workload's shape, against its traffic floor; optionally what scalars() costs with the switch on.

usage: python tools/bench_episode_stats.py [--envs 8192] [--steps 100] [--no-comps] [--reps 20] [--warmup 5] [--scalars]

Kernel time: HIP events around the ABI call (both launches: the scan and the single-workgroup reduce), `warmup` untimed calls, then the
median of `reps`. Floor: the bytes the kernel asks for - reward [T][N] fp32, the reward terms [T][N][12] fp32, and one 64-byte line per
288-byte aux row for the DONE flag (the three height floats are fetched for failures only: not counted) - over the rate this project has
measured for a streaming kernel of its own: adamw_kernel moves 63.05 MB per launch (profiles/pmc_traffic.json) in 15.7 us
(profiles/r06zz_rocprofv3_kernel_stats.md) = 4.02 TB/s. Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stats_bench import STREAM_TBPS, floor_us, timed_call      # noqa: E402 (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--no-comps", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scalars", action="store_true", help="also time task.scalars() with episode_stats off and on (two 8192-env tasks, 3 iterations each)")
    a = ap.parse_args()
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.buffers import TrajBuffers
    from kbot_joystick_amd.spec import compiler, layout as L
    dev = torch.device("cuda", 0)
    T, N = a.steps, a.envs
    ctx = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=N, batch_size=min(N, 512), rollout_len=T))
    traj = TrajBuffers(T, N, 256, 2, dev, reward_comps=not a.no_comps)
    g = torch.Generator(device=dev); g.manual_seed(0)
    traj.reward.uniform_(-1, 2, generator=g)
    if traj.comps is not None:
        traj.comps.uniform_(0, 1, generator=g)
    u = torch.rand(T, N, device=dev, generator=g)
    traj.aux[:T, :, L.AUX["DONE"]] = torch.where(u < 1 / 300, -1.0, torch.where(u < 1 / 150, 1.0, 0.0))     # an episode ends every ~150 steps
    traj.aux[:T, :, L.AUX["BASEZ"]] = torch.rand(T, N, device=dev, generator=g)
    acc = torch.zeros(N, L.EACC["SIZE"], device=dev)
    stats = torch.zeros(L.EPST["SIZE"], dtype=torch.float64, device=dev)
    us, timed = timed_call(lambda: ctx.episode_stats(traj.c, acc, stats), a.reps, a.warmup, "kernel_")
    nbytes = T * N * 4 + (0 if a.no_comps else T * N * 12 * 4) + T * N * 64
    out = dict(envs=N, steps=T, comps=not a.no_comps, **timed, requested_mb=round(nbytes / 1e6, 2), stream_tb_per_s=round(STREAM_TBPS, 2),
               floor_us=round(floor_us(nbytes), 2), ratio=round(us / floor_us(nbytes), 2), episodes_last_call=float(stats[L.EPST["EPISODES"]]))
    ctx.close()
    if a.scalars:
        from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
        for name, on in (("off", False), ("on", True)):
            task = HumanoidWalkingTask(launch_config(num_envs=8192, robot="kbot-headless", fixed_command=(0.5, 0.0, 0.0), seed=0, episode_stats=on))
            t = []
            for _ in range(3):
                task.train_iteration()
                t0 = time.perf_counter(); task.scalars(); t.append((time.perf_counter() - t0) * 1e3)
            out[f"scalars_ms_{name}"] = [round(x, 3) for x in t]
            task.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
