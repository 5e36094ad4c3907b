"""kbj_push_recovery restated on the host (include/kbj.h at kbj_push_recovery; csrc/kbj_push_recovery.h): the per-env scan as a plain loop over
the rows, the group statistics as sequential float64 sums in env order - and a deterministic generator of synthetic problems that holds
every branch of the rule. Shared by tests/test_push_host.py (which asserts, on the CPU, what the problems contain) and tests/test_gpu_push.py.

rec_d holds whole numbers and maxima of the fp32 inputs, so the restatement is compared exactly. The sums: RECOVER_STEPS / FALL_STEPS and their
squares are whole numbers below 2^48, exact in float64 in any order; the peak sums are float64 sums of fp32 values, which depend on the order -
env order here as in the kernel, so they are compared bit for bit too (the square of an fp32 value is exact in float64: a fused multiply-add
changes nothing)."""
from typing import NamedTuple

import numpy as np

from kbot_joystick_amd.spec import layout as L

P, S, O, R, X = L.PREC, L.PSTAT, L.POUT, L.TERR, L.AUX
NE = L.NTERR


def within_rows(err, tol):
    """[T, N] bool: err[t][n][k] <= tol[k] for every error k whose tolerance is not +inf (float32 compares; a NaN is not within; a column with
    a +inf tolerance is not looked at, whatever it holds)."""
    e, tol = np.asarray(err)[:, :, :NE].astype(np.float32), np.asarray(tol, np.float32)
    with np.errstate(invalid="ignore"):
        return ((e <= tol[None, None, :]) | np.isposinf(tol)[None, None, :]).all(-1)


def recovery_ref(err, done, sched, tol, hold, window):
    """rec [N, PREC SIZE] float32, and per env a dict of what the scan met (for the liveness assertions): `broken_run` the longest run a
    not-within row ended, `nan_broke_run` a NaN error ended a run, `by_done` / `by_T` how a CENSORED push was censored."""
    err, done, sched = np.asarray(err, np.float32), np.asarray(done, np.float32), np.asarray(sched, np.int64)
    T, N = done.shape
    ok = within_rows(err, tol)
    rec = np.full((N, P["SIZE"]), -1.0, np.float32)
    diag = []
    for n in range(N):
        s, d = int(sched[n, 0]), max(int(sched[n, 1]), 0)
        info = dict(broken_run=0, nan_broke_run=False, by_done=False, by_T=False)
        diag.append(info)
        if s < 0:
            rec[n, P["OUTCOME"]] = O["NONE"]
            continue
        if s >= T or s < hold or any((not ok[t, n]) or done[t, n] != 0 for t in range(s - hold, s)):
            rec[n, P["OUTCOME"]] = O["VOID"]
            continue
        peak, peak_row, run, outcome = [np.float32(-1.0)] * L.NPEAK, -1.0, 0, None
        for t in range(s, min(T, s + d + window)):
            if err[t, n, R["TILT"]] > peak[R["TILT"]]:
                peak_row = float(t)
            for j in range(L.NPEAK):
                if err[t, n, j] > peak[j]:
                    peak[j] = err[t, n, j]
            if done[t, n] < 0:
                outcome, rec[n, P["FALL_STEPS"]] = O["FELL"], t - s
                break
            if done[t, n] > 0:
                outcome, info["by_done"] = O["CENSORED"], True
                break
            if t >= s + d:
                if ok[t, n]:
                    run += 1
                else:
                    info["broken_run"] = max(info["broken_run"], run)
                    info["nan_broke_run"] |= run > 0 and bool(np.isnan(err[t, n, :NE]).any())
                    run = 0
                if run >= hold:
                    outcome, rec[n, P["RECOVER_STEPS"]] = O["RECOVERED"], (t - hold + 1) - (s + d)
                    break
        if outcome is None:
            info["by_T"] = s + d + window > T
            outcome = O["CENSORED"] if info["by_T"] else O["UNRECOVERED"]
        rec[n, P["OUTCOME"]] = outcome
        rec[n, P["PEAK_LIN"]:P["PEAK_LIN"] + L.NPEAK] = peak
        rec[n, P["PEAK_ROW"]] = peak_row
    return rec, diag


def group_stats_ref(rec, group, G):
    """stats [G, PSTAT SIZE] float64: every group's envs in env order, one float64 add at a time. group None: all in group 0."""
    rec = np.asarray(rec, np.float32)
    st = np.zeros((G, S["SIZE"]), np.float64)
    st[:, [S["REC_MAX"], S["FALL_MAX"]]] = -1.0
    st[:, S["PEAK_MAX"]:S["PEAK_MAX"] + L.NPEAK] = -1.0
    for n in range(rec.shape[0]):
        g = 0 if group is None else int(group[n])
        if not 0 <= g < G:
            continue
        oc = int(rec[n, P["OUTCOME"]])
        st[g, S["COUNT"] + oc] += 1.0
        for which, field in (("REC", "RECOVER_STEPS"), ("FALL", "FALL_STEPS")):
            if oc == O["RECOVERED" if which == "REC" else "FELL"]:
                x = np.float64(rec[n, P[field]])
                st[g, S[which + "_SUM"]] = st[g, S[which + "_SUM"]] + x
                st[g, S[which + "_SUMSQ"]] = st[g, S[which + "_SUMSQ"]] + x * x
                st[g, S[which + "_MAX"]] = max(st[g, S[which + "_MAX"]], x)
        if oc >= O["FELL"]:
            for j in range(L.NPEAK):
                x = np.float64(rec[n, P["PEAK_LIN"] + j])
                st[g, S["PEAK_SUM"] + j] = st[g, S["PEAK_SUM"] + j] + x
                st[g, S["PEAK_MAX"] + j] = max(st[g, S["PEAK_MAX"] + j], x)
    return st


class Problem(NamedTuple):
    err: np.ndarray      # [T, N, TERR SIZE] float32
    aux: np.ndarray      # [T + 1, N, AUX SIZE] float32: only the DONE column is read
    sched: np.ndarray    # [N, 2] int32
    tol: tuple           # five tolerances, one of them +inf
    hold: int
    window: int

    @property
    def done(self):
        return self.aux[:-1, :, X["DONE"]]


TOL, HOLD, WINDOW = (0.5, 0.5, 0.1, float("inf"), 1.0), 3, 8     # the height column is ignored
PATTERNS = 16
SHAPES = [(7, 3), (40, 64), (41, 65), (100, 130)]
# the kernel scans chunks of 8 rows aligned to multiples of 8, two register images in turn: T an exact multiple with three chunks (the last
# image owns row T - 1, the first is used a second time) and the same with a one-row tail
CHUNK_SHAPES = [(24, 65), (25, 70)]
FULL = lambda T, N: T >= 24 and N >= 64      # the shapes that must hold every case three times


def groups(N, G):
    """Every env's group in [0, G); env 1 (when there is one) sits outside and counts in no group."""
    g = ((np.arange(N) * 7 + 3) % G).astype(np.int32)
    if N > 1:
        g[1] = G
    return g


def problems(T, N) -> Problem:
    """Env e holds pattern e % 16 in variant e // 16 (the start row moves with the variant, so the hold rows and windows straddle the chunk
    boundaries differently). Rows that are not written lie within the tolerances; positions outside the trajectory are dropped."""
    rng = np.random.default_rng(1000 * T + N)
    tolf = np.array([t if np.isfinite(t) else 5.0 for t in TOL], np.float32)
    err = np.zeros((T, N, R["SIZE"]), np.float32)
    err[:, :, :NE] = rng.uniform(0.0, 0.9, (T, N, NE)).astype(np.float32) * tolf          # within; the ignored column up to 4.5
    err[:, :, NE:] = rng.uniform(-3.0, 3.0, (T, N, R["SIZE"] - NE)).astype(np.float32)    # mode, settled, since: not read
    aux = np.zeros((T + 1, N, X["SIZE"]), np.float32)
    sched = np.zeros((N, 2), np.int32)

    def out(n, t0, t1, col=R["LIN"], value=None):          # rows [t0, t1) of env n leave the tolerances
        for t in range(max(t0, 0), min(t1, T)):
            err[t, n, col] = np.float32(1.5 + 0.01 * t) * tolf[col] if value is None else value

    def done(n, t, value):
        if 0 <= t < T:
            aux[t, n, X["DONE"]] = value

    for n in range(N):
        p, v = n % PATTERNS, n // PATTERNS
        s, d = 8 + v, 2
        if p == 0:                                   # no push
            s = -1 - v
        elif p == 1:                                 # VOID: a hold row in front of the push is not within
            out(n, s - 2, s - 1, R["YAW"])
        elif p == 2:                                 # FELL two rows into a three-row push
            d = 3; out(n, s, s + 3, R["TILT"]); done(n, s + 2, -1.0)
        elif p == 3:                                 # RECOVERED two rows behind the push
            out(n, s, s + d + 2)
        elif p == 4:                                 # UNRECOVERED: never back
            out(n, s, T)
        elif p == 5:                                 # CENSORED by a time-out before any decision
            out(n, s, T); done(n, s + 3, 1.0)
        elif p == 6:                                 # recovery completes on the window's last row
            out(n, s, s + d + WINDOW - HOLD)
        elif p == 7:                                 # a hold run broken one row short, then never back
            out(n, s, s + d); out(n, s + d + HOLD - 1, T, R["ARM"])
        elif p == 8:                                 # a failure on the first pushed row
            done(n, s, -1.0)
        elif p == 9:                                 # the push comes before `hold` rows exist
            s = v % HOLD
        elif p == 10:                                # the push ends with the trajectory
            d = 2 + v % 2; s = T - d; out(n, s, T)
        elif p == 11:                                # the push starts behind the trajectory
            s = T + v
        elif p == 12:                                # no pushed row at all
            d = 0
        elif p == 13:                                # a NaN error inside a would-be hold run - and, a row on, a NaN in the ignored column, which breaks nothing
            out(n, s + d + 1, s + d + 2, R["YAW"] if v % 2 else R["TILT"], np.float32("nan"))
            out(n, s + d + 2, s + d + 3, R["HEIGHT"], np.float32("nan"))
        elif p == 14:                                # the trajectory cuts the window
            d = 1; s = T - 4 - v % 2; out(n, s, T)
        elif p == 15:                                # VOID: an episode ended on the row in front of the push
            done(n, s - 1, 1.0 if v % 2 else -1.0)
        sched[n] = (s, d)
    return Problem(err, aux, sched, TOL, HOLD, WINDOW)


def contents(prob: Problem) -> dict:
    """How many envs of a problem hold each case of the rule that tests/test_push_host.py asks for three times (counted from the data and the restatement's own scan, not from the pattern ids)."""
    rec, diag = recovery_ref(prob.err, prob.done, prob.sched, prob.tol, prob.hold, prob.window)
    T = prob.done.shape[0]
    oc, s, d = rec[:, P["OUTCOME"]], prob.sched[:, 0], prob.sched[:, 1]
    scanned = oc >= O["FELL"]
    c = {name: int((oc == O[name]).sum()) for name in ("NONE", "VOID", "FELL", "RECOVERED", "UNRECOVERED", "CENSORED")}
    c["recovered_on_last_window_row"] = int(((oc == O["RECOVERED"]) & (rec[:, P["RECOVER_STEPS"]] == prob.window - prob.hold)).sum())
    c["run_broken_one_short"] = sum(x["broken_run"] == prob.hold - 1 for x in diag)
    c["fell_on_row_s"] = int(((oc == O["FELL"]) & (rec[:, P["FALL_STEPS"]] == 0)).sum())
    c["timeout_before_decision"] = sum(x["by_done"] for x in diag)
    c["s_below_hold"] = int(((s >= 0) & (s < prob.hold)).sum())
    c["push_ends_with_T"] = int((scanned & (s + d == T)).sum())
    c["s_behind_T"] = int((s >= T).sum())
    c["d_zero"] = int((scanned & (d == 0)).sum())
    c["nan_in_hold_run"] = sum(x["nan_broke_run"] for x in diag)
    c["window_cut_by_T"] = sum(x["by_T"] for x in diag)
    ignored = [k for k in range(NE) if np.isposinf(np.float32(prob.tol[k]))]
    nan_ign = np.isnan(prob.err[:, :, ignored]).any(-1) & ~np.isnan(np.delete(prob.err[:, :, :NE], ignored, axis=2)).any(-1)
    c["nan_in_ignored_column_inside_a_recovery_run"] = int(sum(                  # a NaN the +inf tolerance hides, on a row of the run that recovers
        oc[n] == O["RECOVERED"] and nan_ign[int(s[n] + d[n] + rec[n, P["RECOVER_STEPS"]]):int(s[n] + d[n] + rec[n, P["RECOVER_STEPS"]]) + prob.hold, n].any()
        for n in range(len(s))))
    return c
