"""kbj_robustness alone at a sweep's length and a wide env count, with and without the group statistics, against its traffic floor, and
kbj_env_perturb at the same env count.

usage: python tools/bench_robustness.py [--envs 4096] [--steps 500] [--groups 64] [--reps 20] [--warmup 5]

Shape: T = 500 rows (10 s at ctrl_dt = 0.02 s), N = 4096 envs in G = 64 cases. Synthetic err rows (errors of mixed scale, most rows
settled) and aux rows with an episode end every ~300 steps. The scan reads every row of every env, whatever it holds.
Kernel time: HIP events around the ABI call (the scan and, with stats_d, the single-workgroup second stage), `warmup` untimed calls, then
the median of `reps`. Floor: the bytes a call needs - 36 per (row, env): the 32-byte err row and the DONE word of the aux row - plus the
records it writes (and, with stats_d, reads again), at the copy rate measured in the SAME process (a device-to-device copy of 256 MiB, read
plus write). The DONE words lie 288 bytes apart, so the hardware moves more than the floor counts. kbj_env_perturb: every env masked, a valid
record each; its floor is the record read and the 346 words written per env. Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stats_bench import timed_call      # noqa: E402 (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.robustness import default_perturbations
    from kbot_joystick_amd.spec import compiler, layout as L
    dev = torch.device("cuda", 0)
    T, N, G = a.steps, a.envs, a.groups
    X, R, S, TE = L.AUX, L.RREC, L.RSTAT, L.TERR
    # the copy rate of this process, on this device, now
    src, dst = torch.empty(64 << 20, device=dev), torch.empty(64 << 20, device=dev)
    copy_us, _ = timed_call(lambda: dst.copy_(src), a.reps, a.warmup)
    copy_tbps = 2 * src.numel() * 4 / copy_us / 1e6
    del src, dst
    floor = lambda nbytes: nbytes / (copy_tbps * 1e12) * 1e6
    out = dict(copy_tb_per_s=round(copy_tbps, 2), T=T, N=N, G=G)

    ctx = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=N, batch_size=min(512, N), hidden_size=64, rollout_len=8))
    g = torch.Generator(device=dev); g.manual_seed(0)
    aux = torch.rand(T + 1, N, X["SIZE"], device=dev, generator=g) - 0.5
    u = torch.rand(T + 1, N, device=dev, generator=g)
    aux[:, :, X["DONE"]] = torch.where(u < 1 / 600, -1.0, torch.where(u < 1 / 300, 1.0, 0.0))
    err = torch.rand(T, N, TE["SIZE"], device=dev, generator=g)
    err[:, :, TE["SETTLED"]] = (torch.rand(T, N, device=dev, generator=g) < 0.8).float()
    rec = torch.zeros(N, R["SIZE"], dtype=torch.float64, device=dev)
    stats = torch.zeros(G, S["SIZE"], dtype=torch.float64, device=dev)
    group = (torch.arange(N, device=dev) % G).to(torch.int32)
    traj = B.Traj(T=T, N=N, aux_d=aux.data_ptr())
    scan_bytes = T * N * 36 + N * R["SIZE"] * 8
    for leg, st, nbytes in (("rec_only", None, scan_bytes), ("with_stats", stats, scan_bytes + N * (R["SIZE"] * 8 + 4) + G * S["SIZE"] * 8)):
        res = timed_call(lambda: ctx.robustness(traj, err, rec, group, G, st), a.reps, a.warmup)[1]
        res.update(needed_mb=round(nbytes / 1e6, 3), floor_us=round(floor(nbytes), 3))
        res["ratio_to_floor"] = round(res["us_median"] / res["floor_us"], 1)
        out[leg] = res
    r = rec.cpu().numpy()
    out["falls"], out["settled_rows"] = int(r[:, R["FALLS"]].sum()), int(r[:, R["SETTLED"]].sum())

    cases = default_perturbations()
    pert = torch.from_numpy(np.stack([cases[e % len(cases)].record() for e in range(N)])).to(dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    obs = (torch.zeros(N, L.LD_ACTOR, device=dev), torch.zeros(N, L.LD_CRITIC, device=dev), torch.zeros(N, X["SIZE"], device=dev))
    ctx.env_reset_all(1, *obs)
    res = timed_call(lambda: ctx.env_perturb(None, pert, status), a.reps, a.warmup)[1]
    nbytes = N * (L.PERT["SIZE"] * 4 + (L.EP["MU"] + 1) * 4 + 4)
    res.update(needed_mb=round(nbytes / 1e6, 3), floor_us=round(floor(nbytes), 3), written=int((status == 1).sum()))
    out["env_perturb"] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
