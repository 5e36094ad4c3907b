"""kbj_frequency_response alone at a sweep's length and a wide env count, with and without the group statistics, against its traffic floor and
beside kbj_step_response on the same rows.

usage: python tools/bench_frequency_response.py [--envs 8192] [--steps 550] [--reps 20] [--warmup 5]

Shape: T = 550 rows, N envs in G = 15 cases = 3 channels x the periods 100, 48, 24, 12 and 8 rows; the sinusoid starts on row 50, a case measures
K = max(4, ceil(200 / P)) whole periods from row s = 50 + ceil(50 / P) P (task.frequency_sweep()'s rule with start_at = settle = 1 s and
min_window = 4 s at ctrl_dt = 0.02 s). Synthetic aux rows: the driven command word is 0.5 cos, the response a scaled copy a few rows late
with a little noise under random attitudes. Leg `follows`: no episode ends, every lane walks its quarter period of lead rows and its whole
window. Leg `falls`: an episode end every ~300 steps per env, so many scans stop early and some windows are VOID.
Kernel time: HIP events around the ABI call (the signal kernel, the scan and, with stats_d, the single-workgroup second stage), `warmup`
untimed calls, then the median of `reps`. Floor: the bytes a call needs - for every row the 14 aux words stage 1 reads and the 32 bytes it
writes, for every env the signal rows [s - q, last scanned row] re-read at 32 bytes, its schedule row and its record - over the rate this
project has measured for a streaming kernel of its own (tools/stats_bench.py). The aux words of a row lie in three places of its 288 bytes,
so the hardware moves more than the floor counts. `step_response`: kbj_step_response (rec only) on the same aux rows with the step
scheduled on each env's s and task.step_sweep()'s default criteria - the same stage 1, another scan. Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stats_bench import STREAM_TBPS, floor_us, timed_call      # noqa: E402 (tools/ is the script's directory)

PERIODS = (100, 48, 24, 12, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=550)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.frequency import case_schedule
    from kbot_joystick_amd.spec import compiler, layout as L
    dev = torch.device("cuda", 0)
    ctx = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=64, batch_size=64, hidden_size=64, rollout_len=8))
    X, R, S, O = L.AUX, L.FREC, L.FSTAT, L.FOUT
    T, N, start = a.steps, a.envs, 50
    cases = [(ch, P) + case_schedule(P, 0.02, 4, 4.0, start, 50) for ch in range(3) for P in PERIODS]
    G = len(cases)
    assert max(s + K * P for _, P, s, K in cases) <= T, "--steps is too short for the slowest case"
    case = np.arange(N) % G
    sched_h = np.array([[cases[c][2], cases[c][1], cases[c][0], cases[c][3]] for c in case], np.int32)
    out = dict(stream_tb_per_s=round(STREAM_TBPS, 2), T=T, N=N, G=G, periods=list(PERIODS), start_row=start)
    sched = torch.from_numpy(sched_h).to(dev)
    group = torch.from_numpy(case.astype(np.int32)).to(dev)
    crit = B.FrequencyCriteria((B.C.c_float * L.NSCH)(0.05, 0.05, 0.05))
    f3 = B.C.c_float * L.NSCH
    step_crit = B.StepCriteria(f3(0.05, 0.05, 0.05), f3(0.15, 0.15, 0.25), 0.1, 0.9, 25, 25, 200)
    step_sched = sched[:, 0].contiguous()
    sig = torch.zeros(T, N, L.SSIG["SIZE"], device=dev)
    rec = torch.zeros(N, R["SIZE"], dtype=torch.float64, device=dev)
    step_rec = torch.zeros(N, L.SREC["SIZE"], device=dev)
    stats = torch.zeros(G, S["SIZE"], dtype=torch.float64, device=dev)
    P_env, ch_env = torch.from_numpy(sched_h[:, 1]).to(dev).float(), torch.from_numpy(sched_h[:, 2]).to(dev).long()
    envs = torch.arange(N, device=dev)
    for name, every in (("follows", None), ("falls", 300)):
        g = torch.Generator(device=dev); g.manual_seed(0)
        aux = torch.rand(T + 1, N, X["SIZE"], device=dev, generator=g) - 0.5
        yaw = torch.rand(T + 1, N, device=dev, generator=g) * 6.2831853
        aux[:, :, X["BQUAT"]], aux[:, :, X["BQUAT"] + 3] = torch.cos(0.5 * yaw), torch.sin(0.5 * yaw)
        aux[:, :, X["BQUAT"] + 1:X["BQUAT"] + 3] *= 0.05
        k = (torch.arange(T + 1, device=dev, dtype=torch.float32) - start).clamp(min=0)[:, None]
        theta = 6.2831853 * k / P_env[None, :]
        aux[:, :, X["CMD"]:X["CMD"] + L.NCMD] = 0.0
        aux[:, envs, X["CMD"] + ch_env] = 0.5 * torch.cos(theta)
        v = 0.4 * torch.cos(theta - 0.6) + 0.02 * (torch.rand(T + 1, N, device=dev, generator=g) - 0.5)      # a scaled copy, late by 0.6 rad
        aux[:, :, X["QVEL"]], aux[:, :, X["QVEL"] + 1] = torch.cos(yaw) * v, torch.sin(yaw) * v      # v along the heading
        aux[:, :, X["QVEL"] + 5] = v
        if every:
            u = torch.rand(T + 1, N, device=dev, generator=g)
            aux[:, :, X["DONE"]] = torch.where(u < 0.5 / every, -1.0, torch.where(u < 1.0 / every, 1.0, 0.0))
        else:
            aux[:, :, X["DONE"]] = 0.0
        traj = B.Traj(T=T, N=N, aux_d=aux.data_ptr())
        res = {}
        for leg, st in (("rec_only", None), ("with_stats", stats)):
            res[leg] = timed_call(lambda: ctx.frequency_response(traj, sched, crit, sig, rec, group, G, st), a.reps, a.warmup)[1]
        res["step_response"] = timed_call(lambda: ctx.step_response(traj, step_sched, step_crit, sig, step_rec), a.reps, a.warmup)[1]
        r = rec.cpu().numpy()
        oc = r[:, R["OUTCOME"]].astype(int)
        # the rows an env's lane re-reads: its lead rows, then up to the row that stopped it (VOID on a lead row: counted in full, an upper bound)
        scanned = [sched_h[n, 1] // 4 + (int(x[R["ROWS"]]) + (o in (O["FELL"], O["CENSORED"])) if o >= O["FELL"] else 0) for n, (x, o) in enumerate(zip(r, oc))]
        nbytes = T * N * (14 * 4 + L.SSIG["SIZE"] * 4) + int(sum(scanned)) * L.SSIG["SIZE"] * 4 + N * (16 + R["SIZE"] * 8)
        res.update(needed_mb=round(nbytes / 1e6, 3), floor_us=round(floor_us(nbytes), 3), outcomes=[int((oc == i).sum()) for i in range(O["COUNT"])])
        for leg in ("rec_only", "with_stats"):
            res[leg]["ratio_to_floor"] = round(res[leg]["us_median"] / res["floor_us"], 1)
        out[name] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
