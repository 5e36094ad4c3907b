"""kbj_actuator_stats alone at the workload's shape, with and without the per-env record, beside kbj_gait_stats on the same rows in the same
run, against its traffic floor.

usage: python tools/bench_actuator_stats.py [--envs 8192] [--steps 100] [--reps 20] [--warmup 5]

Kernel time: HIP events around the ABI call (both launches: the scan and the wide reduce), `warmup` untimed calls, then the median of `reps`;
the kernel records of the library split one more call into its two launches. Floor: the bytes the scan reads per row - the 29 16-byte pieces
of kbj_actuator_stats.h: 12 of the aux row, 12 of the state record, 5 of the action row, 464 bytes - times the rows, over the copy bandwidth
measured here, in the same process: a device-to-device copy of 512 MB, read plus write, median of `reps`. The partials the scan writes and
the reduce reads (blocks x 1792 doubles, twice) are reported beside it, not in it. Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stats_bench import timed_call      # noqa: E402 (tools/ is the script's directory)

ROW_BYTES = 29 * 16
ENVS_PER_BLOCK = 16                     # kbj_actuator_stats.h ACT_ENVS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from kbot_joystick_amd.host import actuator as HA, binding as B
    from kbot_joystick_amd.spec import compiler, layout as L
    dev = torch.device("cuda", 0)
    T, N = a.steps, a.envs
    model = compiler.load_model("kbot-headless")
    ctx = B.Context(model, L.default_config(num_envs=N, batch_size=min(N, 512), rollout_len=T))
    g = torch.Generator(device=dev); g.manual_seed(0)
    X, Q = L.AUX, L.QSTATE
    aux = torch.rand(T + 1, N, X["SIZE"], device=dev, generator=g) * 2 - 1
    cmd = torch.zeros(T, N, L.NCMD, device=dev)
    modes = torch.randint(0, 6, (N,), device=dev, generator=g)                      # one command per env and call, a sixth of the envs per mode
    cmd[:, modes == 0, 0], cmd[:, modes == 1, 1], cmd[:, modes == 2, 2] = 0.7, 0.3, 0.5
    cmd[:, modes == 3, :3], cmd[:, modes == 3, 6] = 0.4, 0.3
    cmd[:, modes == 4, 3] = -0.1
    cmd[T // 2:, : N // 4, 0] += 0.1                                                  # a quarter of the envs switch mid-way
    aux[:T, :, X["CMD"]:X["CMD"] + L.NCMD] = cmd
    u = torch.rand(T, N, device=dev, generator=g)
    aux[:T, :, X["DONE"]] = torch.where(u < 1 / 300, -1.0, torch.where(u < 1 / 150, 1.0, 0.0))     # an episode ends every ~150 steps
    aux[:T, :, X["TOUCH"]:X["TOUCH"] + 2] = aux[:T, :, X["TOUCH"]:X["TOUCH"] + 2].abs() * 300.0
    aux[:T, :, X["CTRL"]:X["CTRL"] + L.NU] *= torch.tensor(list(model.tau_limit), device=dev)      # torques up to the limit: some rows at the 0.9 level
    qstate = torch.rand(T, N, Q["SIZE"], device=dev, generator=g) * 4 - 2
    action = torch.rand(T, N, L.NU, device=dev, generator=g) - 0.5
    traj = B.Traj(T=T, N=N, aux_d=aux.data_ptr(), qstate_d=qstate.data_ptr(), action_d=action.data_ptr())
    lv = HA.actuator_levels(model, speed_limit=1.5)
    # the copy bandwidth of this device, in this process
    src = torch.empty(512 * 1024 * 1024 // 4, device=dev).normal_(generator=g)
    dst = torch.empty_like(src)
    copy_us, copy = timed_call(lambda: dst.copy_(src), a.reps, a.warmup, "copy_")
    tbps = 2 * src.numel() * 4 / copy_us / 1e6
    nbytes = T * N * ROW_BYTES
    floor = nbytes / (tbps * 1e12) * 1e6
    blocks = (N + ENVS_PER_BLOCK - 1) // ENVS_PER_BLOCK
    out = dict(envs=N, steps=T, copy_tb_per_s=round(tbps, 2), **copy, read_mb=round(nbytes / 1e6, 2), floor_us=round(floor, 2), partials_mb=round(blocks * L.ACT["SIZE"] * 8 / 1e6, 2))
    acc, stats, env = torch.zeros(N, L.AACC["SIZE"], device=dev), torch.zeros(L.ACT["SIZE"], dtype=torch.float64, device=dev), torch.zeros(N, L.AENV["SIZE"], device=dev)
    gacc, gstats = torch.zeros(N, L.GACC["SIZE"], device=dev), torch.zeros(L.GAIT["SIZE"], dtype=torch.float64, device=dev)
    calls = (("actuator_stats_only", lambda: ctx.actuator_stats(traj, lv, acc, stats)), ("actuator_with_env", lambda: ctx.actuator_stats(traj, lv, acc, stats, env)),
             ("gait_stats_only", lambda: ctx.gait_stats(traj, gacc, gstats)))
    for name, call in calls:
        us, out[name] = timed_call(call, a.reps, a.warmup, "kernel_")
        out[name]["ratio_to_floor"] = round(us / floor, 2)
    ctx.profile_begin()
    ctx.actuator_stats(traj, lv, acc, stats)
    out["launches_us"] = {k["name"]: round(k["total_ms"] * 1e3, 2) for k in ctx.profile_end()["kernels"]}
    v = stats.cpu().numpy()
    out["rows_per_mode"] = [float(v[L.act_slot(m, "ROWS")]) for m in range(L.CMODE["COUNT"])]
    out["any_tau_rows"] = float(sum(v[L.act_slot(m, "ANY_TAU_ROWS")] for m in range(L.CMODE["COUNT"])))
    out["pairs"] = float(sum(v[L.act_slot(m, "PAIRS")] for m in range(L.CMODE["COUNT"])))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
