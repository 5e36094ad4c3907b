"""kbj_actuator_stats restated in numpy with the kernel's arithmetic (include/kbj.h: fp32 row quantities, float64 sums, fixed orders), and the
synthetic problems the host and GPU tests share. No GPU, no library."""
import functools
import math

import numpy as np

from kbot_joystick_amd.spec import layout as L
from tests.gait_ref import _prototypes, mode_of

f32 = np.float32
V, J, A, E, X, Q, M = L.ACT, L.AJNT, L.AACC, L.AENV, L.AUX, L.QSTATE, L.CMODE
NU = L.NU
ENVS, CHUNK = 16, 4                               # kbj_actuator_stats.h ACT_ENVS (envs per workgroup) and ACT_TC (rows per staging chunk)
SHAPES = [(1, 1), (5, ENVS - 1), (6, ENVS), (7, ENVS + 1), (3 * CHUNK - 1, 2 * ENVS + 1), (3 * CHUNK + 1, ENVS + 1)]
REAL_SUMS = ("TAU_SQ", "VEL_SQ", "POW_ABS", "POW_POS", "DACT_SQ")     # joint slots that are double sums of real values; SPEED_SUM is the head slot
COUNTS = ("TAU_ROWS", "VEL_ROWS", "STOP_ROWS")
LEVEL_NAMES = ("tau_level", "vel_level", "pos_lo", "pos_hi")


def slot(mode, name, joint=None):
    return L.act_slot(mode, name, joint)


def synthetic_levels() -> dict:
    """Levels that differ across all 20 joints; the odd joints have no speed level (+inf)."""
    u = np.arange(NU)
    return dict(tau_level=(10.0 + 3.0 * u).astype(f32), vel_level=np.where(u % 2 == 1, np.inf, 2.0 + 0.5 * u).astype(f32),
                pos_lo=(-1.0 - 0.05 * u).astype(f32), pos_hi=(1.0 + 0.03 * u).astype(f32))


def c_levels(lv):
    """The levels as the ABI's struct."""
    from kbot_joystick_amd.host import binding as B
    out = B.ActuatorLevels()
    for k in LEVEL_NAMES:
        for j in range(NU):
            getattr(out, k)[j] = float(lv[k][j])
    return out


def levels_dict(c) -> dict:
    """An ABI struct as the float32 arrays actuator_ref takes."""
    return {k: np.array(list(getattr(c, k)), f32) for k in LEVEL_NAMES}


def actuator_ref(acc, aux, qstate, action, T, lv):
    """kbj_actuator_stats on rows 0 .. T-1 of aux [>= T, N, 72], qstate [>= T, N, 80] and action [>= T, N, 20] (float32) with the carry rows
    acc [N, AACC SIZE] float32, updated in place. Returns (stats, mags, env): the KBJ_ACT vector with every real-valued sum taken by
    math.fsum, per slot the sum of |x| of what such a sum adds up (0 elsewhere), and the per-env record [N, AENV SIZE] float32 with the
    kernel's own order: per (env, actuator) a float64 sum over the rows in ascending t, the 20 actuators added in ascending u from 0.0,
    rounded to fp32 once."""
    aux, qstate, action = (np.asarray(x, f32)[:T] for x in (aux, qstate, action))
    N = aux.shape[1]
    tau = aux[:, :, X["CTRL"]:X["CTRL"] + NU]
    om, q = qstate[:, :, Q["QVEL"] + 6:Q["QVEL"] + 6 + NU], qstate[:, :, Q["QPOS"] + 7:Q["QPOS"] + 7 + NU]
    assert tau.dtype == om.dtype == q.dtype == action.dtype == f32
    P = tau * om                                                    # one fp32 product
    mode = np.array([[mode_of(aux[t, n, X["CMD"]:X["CMD"] + L.NCMD]) for n in range(N)] for t in range(T)]).reshape(T, N)
    open_ = aux[:, :, X["DONE"]] == 0
    pair = np.concatenate([acc[None, :, A["RUNNING"]] != 0, open_[:-1]])                  # [T, N]: the row before belongs to the same episode
    d = action - np.concatenate([acc[None, :, A["PREV"]:A["PREV"] + NU], action[:-1]])    # fp32
    vx, vy = aux[:, :, X["QVEL"]].astype(np.float64), aux[:, :, X["QVEL"] + 1].astype(np.float64)
    speed = np.sqrt(vx * vx + vy * vy)
    atau, aom, aP = np.abs(tau), np.abs(om), np.abs(P)
    at_tau, over, at_stop = atau >= lv["tau_level"], aom >= lv["vel_level"], (q <= lv["pos_lo"]) | (q >= lv["pos_hi"])
    x64 = lambda a: a.astype(np.float64)
    real = dict(TAU_SQ=x64(tau) * x64(tau), VEL_SQ=x64(om) * x64(om), POW_ABS=x64(aP), POW_POS=x64(np.maximum(P, f32(0))), DACT_SQ=np.where(pair[:, :, None], x64(d) * x64(d), 0.0))
    tops = dict(TAU_MAX=atau, VEL_MAX=aom, POW_MAX=aP, DACT_MAX=np.where(pair[:, :, None], np.abs(d), f32(0)))
    counts = dict(TAU_ROWS=at_tau, VEL_ROWS=over, STOP_ROWS=at_stop)
    stats, mags = np.zeros(V["SIZE"]), np.zeros(V["SIZE"])
    for m in range(M["COUNT"]):
        sel = mode == m
        if not sel.any():
            continue
        stats[slot(m, "ROWS")], stats[slot(m, "PAIRS")] = sel.sum(), (sel & pair).sum()
        stats[slot(m, "ANY_TAU_ROWS")], stats[slot(m, "ANY_STOP_ROWS")] = (sel & at_tau.any(2)).sum(), (sel & at_stop.any(2)).sum()
        xs = speed[sel].tolist()
        stats[slot(m, "SPEED_SUM")], mags[slot(m, "SPEED_SUM")] = math.fsum(xs), math.fsum(xs)
        for u in range(NU):
            for k, x in real.items():
                xs = x[:, :, u][sel & pair] if k == "DACT_SQ" else x[:, :, u][sel]
                stats[slot(m, k, u)], mags[slot(m, k, u)] = math.fsum(xs.tolist()), math.fsum(np.abs(xs).tolist())
            for k, x in tops.items():
                stats[slot(m, k, u)] = np.fmax.reduce(x[:, :, u][sel], initial=f32(0))
            for k, x in counts.items():
                stats[slot(m, k, u)] = x[:, :, u][sel].sum()
    stats[V["EPISODES"]] = (~pair).sum()
    # the per-env record: sequential float64 sums (np.cumsum adds in order), rows first, then the actuators
    seq = lambda x: np.cumsum(np.cumsum(x, axis=0)[-1], axis=-1)[..., -1]                 # [T, N, NU] -> [N]
    env = np.zeros((N, E["SIZE"]), f32)
    env[:, E["ROWS"]], env[:, E["PAIRS"]] = T, pair.sum(0)
    env[:, E["SPEED_SUM"]] = np.cumsum(speed, axis=0)[-1].astype(f32)
    for k in ("TAU_SQ", "POW_ABS", "POW_POS", "DACT_SQ"):
        env[:, E[k]] = seq(real[k]).astype(f32)
    env[:, E["ANY_TAU_ROWS"]], env[:, E["ANY_STOP_ROWS"]] = at_tau.any(2).sum(0), at_stop.any(2).sum(0)
    peak = np.fmax.reduce(atau / lv["tau_level"], axis=0, initial=f32(0))                 # [N, NU] fp32 divisions
    env[:, E["PEAK_FRAC"]], env[:, E["PEAK_JOINT"]] = peak.max(1), peak.argmax(1)         # argmax: the lowest u on a tie
    acc[:, A["PREV"]:A["PREV"] + NU], acc[:, A["RUNNING"]] = action[T - 1], open_[T - 1]
    return stats, mags, env


def exact_slots():
    """The slots of a KBJ_ACT vector that hold whole numbers or fp32 maxima: all but the real-valued sums."""
    m = np.ones(V["SIZE"], bool)
    for mode in range(M["COUNT"]):
        m[slot(mode, "SPEED_SUM")] = False
        for u in range(NU):
            for k in REAL_SUMS:
                m[slot(mode, k, u)] = False
    return m


def used_slots():
    m = np.zeros(V["SIZE"], bool)
    for mode in range(M["COUNT"]):
        m[mode * V["MODE_STRIDE"]:mode * V["MODE_STRIDE"] + 5] = True
        m[mode * V["MODE_STRIDE"] + V["JOINT"]:mode * V["MODE_STRIDE"] + V["JOINT"] + NU * J["SIZE"]] = True
    m[V["EPISODES"]] = True
    return m


def assert_stats_match(got, want, mags):
    """Counts and maxima exact; the double sums of real values within 1e-9 * sum |x| of math.fsum (the margin tests/test_gpu_episode_stats.py
    derives for double accumulation in any order); unused slots 0."""
    ex = exact_slots()
    assert np.array_equal(got[ex], want[ex]), np.flatnonzero(ex)[got[ex] != want[ex]]
    assert (np.abs(got[~ex] - want[~ex]) <= 1e-9 * mags[~ex]).all(), (got[~ex], want[~ex])
    assert (got[~used_slots()] == 0).all()


# ---- synthetic problems ----
class Problems:
    """Two consecutive calls of one shape: `calls[i]` = (aux [T + 1, N, 72], qstate [T, N, 80], action [T, N, 20]) float32 of call i (aux row
    T is never read: it holds 1e9), `acc0` the carry the first call starts from (zeros, the spare floats 7.0), `lv` the levels
    (synthetic_levels). Every column the kernel does not read holds noise; torque, speed, position and action are random with a scale
    that differs per joint; every env holds a command of each mode by turns, changed now and then inside an episode; episodes end on 8 % of
    the rows with either sign. With T >= 5 and N >= 10 the first envs are scripted instead, over the 2 T rows r of both calls:
      env 0: DONE = -1 on row 0.                          env 1: DONE = +1 on row 0.
      env 2: DONE = -1 on row T - 1: the pair across the call boundary is cut.
      env 3: DONE = 0 on row T - 1: that pair is kept; DONE = +1 on row 2 T - 1.
      env 4: DONE = -1 on row 1 and +1 on row 2: consecutive ends.
      env 5: row 1 has every |tau|, |omega| exactly ON its level (signs alternate) and q exactly on pos_lo (even u) / pos_hi (odd u); row 2 has
             them one fp32 step inside (nextafter towards 0 / towards the middle): not counted.
      env 6: row 1 holds -0.0 in torque, speed, action and in the command's first component (still a zero command); row 2 holds -0.0 speeds
             against +1 torques (P = -0.0).
      env 7: small torques but for row 2 and row T + 2, where joints 3 and 11 both sit at exactly twice their level: a PEAK_JOINT tie, 3 wins.
      env 8: the carry says RUNNING with a previous action: row 0 has a pair."""

    def __init__(self, T, N):
        rng = np.random.default_rng(2000 * T + N)
        R, lv = 2 * T, synthetic_levels()
        done = np.where(rng.random((R, N)) < 0.08, rng.choice([-1.0, 1.0], (R, N)), 0.0).astype(f32)
        cmd = np.zeros((R, N, L.NCMD), f32)
        for n in range(N):
            protos = _prototypes(rng)
            mode, r = (n + int(rng.integers(0, 2))) % M["COUNT"], 0
            while r < R:
                hold = int(rng.integers(2, R + 2))
                cmd[r:r + hold, n] = protos[mode]
                mode, r = int(rng.integers(0, M["COUNT"])), r + hold
        scale = 1.0 + 0.25 * np.arange(NU)
        tau = (rng.standard_normal((R, N, NU)) * 0.6 * lv["tau_level"]).astype(f32)
        om = (rng.standard_normal((R, N, NU)) * 1.5 * scale).astype(f32)
        q = (rng.standard_normal((R, N, NU)) * 0.7).astype(f32)
        act = (rng.standard_normal((R, N, NU)) * 0.1 * scale).astype(f32)
        self.acc0 = np.zeros((N, A["SIZE"]), f32)
        self.acc0[:, A["RUNNING"] + 1:] = 7.0
        planted = T >= 5 and N >= 10
        if planted:
            done[:, :9] = 0.0
            done[0, 0], done[0, 1], done[T - 1, 2], done[R - 1, 3], done[1, 4], done[2, 4] = -1.0, 1.0, -1.0, 1.0, -1.0, 1.0
            sign = np.where(np.arange(NU) % 2 == 0, 1.0, -1.0).astype(f32)
            finite = np.where(np.isfinite(lv["vel_level"]), lv["vel_level"], f32(3.0))
            tau[1, 5], om[1, 5], q[1, 5] = sign * lv["tau_level"], -sign * finite, np.where(sign > 0, lv["pos_lo"], lv["pos_hi"])
            tau[2, 5], om[2, 5] = sign * np.nextafter(lv["tau_level"], f32(0)), -sign * np.nextafter(finite, f32(0))
            q[2, 5] = np.where(sign > 0, np.nextafter(lv["pos_lo"], f32(0)), np.nextafter(lv["pos_hi"], f32(0)))
            tau[1, 6], om[1, 6], act[1, 6], cmd[:, 6] = f32(-0.0), f32(-0.0), f32(-0.0), 0.0
            cmd[1, 6, 0] = f32(-0.0)
            tau[2, 6], om[2, 6] = f32(1.0), f32(-0.0)
            tau[:, 7] = (rng.uniform(-0.5, 0.5, (R, NU)) * lv["tau_level"]).astype(f32)
            for r in (2, T + 2):
                tau[r, 7, 3], tau[r, 7, 11] = f32(2.0) * lv["tau_level"][3], f32(-2.0) * lv["tau_level"][11]
            self.acc0[8, A["RUNNING"]], self.acc0[8, A["PREV"]:A["PREV"] + NU] = 1.0, act[0, 8] + f32(0.25)
        aux = rng.standard_normal((R, N, X["SIZE"])).astype(f32)
        aux[:, :, X["CTRL"]:X["CTRL"] + NU], aux[:, :, X["CMD"]:X["CMD"] + L.NCMD], aux[:, :, X["DONE"]] = tau, cmd, done
        qs = rng.standard_normal((R, N, Q["SIZE"])).astype(f32) * 5
        qs[:, :, Q["QPOS"] + 7:Q["QPOS"] + 7 + NU], qs[:, :, Q["QVEL"] + 6:Q["QVEL"] + 6 + NU] = q, om
        self.T, self.N, self.planted, self.lv = T, N, planted, lv
        self.calls = [(np.concatenate([aux[i * T:(i + 1) * T], np.full((1, N, X["SIZE"]), 1e9, f32)]), qs[i * T:(i + 1) * T].copy(), act[i * T:(i + 1) * T].copy()) for i in range(2)]


@functools.lru_cache(maxsize=None)
def problems(T, N):
    return Problems(T, N)


@functools.lru_cache(maxsize=None)
def reference(T, N):
    """The restatement on both calls of problems(T, N), computed once: a list of (acc before, acc after, stats, mags, env) per call. Shared by
    the tests; nobody writes to it."""
    P = problems(T, N)
    acc, out = P.acc0.copy(), []
    for aux, qs, act in P.calls:
        before = acc.copy()
        stats, mags, env = actuator_ref(acc, aux, qs, act, T, P.lv)
        out.append((before, acc.copy(), stats, mags, env))
    return out
