"""kbj_frequency_response restated on the host (include/kbj.h at kbj_frequency_response; csrc/kbj_frequency_response.h): stage 2 as a plain walk over
the rows of a GIVEN fp32 signal - fp32 comparisons for R_MIN / R_MAX and the swing, every sum a float64 cumsum from 0.0 in ascending t (a
cumsum adds one element after the other; np.sum does not) -, the group statistics as sequential float64 operations in env order, the host
formulas of host/frequency.py once more (here through numpy's linear solve) - and a deterministic generator of synthetic aux rows that holds
every branch of the rule. Stage 1 is kbj_step_response's (tests/step_response_ref.py signal_ref). Shared by tests/test_frequency_ref.py (which
asserts, on the CPU, what the problem contains) and the GPU tests.

Everything behind stage 1 holds whole numbers, fp32 extrema, one fp32 subtraction and float64 sums in a fixed order whose products are exact:
it is compared bit for bit, except that a NaN is only asked to be a NaN (an invalid operation's NaN has no agreed sign)."""
from typing import NamedTuple

import numpy as np

from kbot_joystick_amd.spec import layout as L
from tests.step_response_ref import groups, heading64, signal_ref      # noqa: F401 (groups, signal_ref: re-exported for the tests)

G_, R, S, O, X = L.SSIG, L.FREC, L.FSTAT, L.FOUT, L.AUX
NCH, NSUMS = L.NSCH, L.FREC_NSUMS
f32, f64 = np.float32, np.float64
INT32_MAX = 2 ** 31 - 1


def _ordered_sum(x):
    """0.0 + x[0] + x[1] + ..., one float64 add after the other."""
    return np.cumsum(np.concatenate(([0.0], np.asarray(x, f64))))[-1]


# ---- stage 2 ----
def scan_ref(sig, sched, min_amp):
    """rec [N, FREC SIZE] float64 from an fp32 signal [T, N, SSIG SIZE] and a schedule [N, 4] (s, P, ch, K), and per env a dict of what the scan
    met. Python integers throughout: no index overflows."""
    sig = np.asarray(sig, f32)
    T, N = sig.shape[:2]
    min_amp = np.asarray(min_amp, f32)
    rec = np.full((N, R["SIZE"]), -1.0, f64)
    diag = []
    for n in range(N):
        s, P, ch, K = (int(x) for x in sched[n])
        info = dict(void_why=None, by_done=False, by_T=False, stop_row=None, nan_y=False, nan_r=False, on_amp=False)
        diag.append(info)
        if s < 0:
            rec[n, R["OUTCOME"]] = O["NONE"]
            continue
        rec[n, R["OUTCOME"]] = O["VOID"]
        q = P // 4
        for why, bad in (("period", P < 4 or P > 256 or P % 4 != 0), ("channel", not 0 <= ch <= 2), ("cycles", K < 1), ("lead", s < q), ("outside", s >= T)):
            if bad:
                info["void_why"] = why
                break
        if info["void_why"]:
            continue
        if (sig[s - q:s, n, G_["DONE"]] != 0).any():
            info["void_why"] = "lead_done"
            continue
        end = min(T, s + K * P)
        done = sig[s:end, n, G_["DONE"]]
        stops = np.flatnonzero(done != 0)
        stop = s + int(stops[0]) if stops.size else None
        last = stop if stop is not None else end                       # rows [s, last) are accumulated
        r = sig[s:last, n, G_["CMD"] + ch]
        d = sig[s - q:last - q, n, G_["CMD"] + ch]
        y = sig[s:last, n, :NCH]
        rmin, rmax = f32(np.inf), f32(-np.inf)
        for v in r:                                                    # replaced where smaller / greater: a NaN never replaces
            if v < rmin:
                rmin = v
            if v > rmax:
                rmax = v
        if stop is not None:
            outcome = O["FELL"] if sig[stop, n, G_["DONE"]] < 0 else O["CENSORED"]
            info["by_done"], info["stop_row"] = outcome == O["CENSORED"], stop - s
        elif s + K * P > T:
            outcome, info["by_T"] = O["CENSORED"], True
        else:
            with np.errstate(invalid="ignore"):
                swing = f32(rmax - rmin)
                outcome = O["MEASURED"] if swing >= min_amp[ch] else O["FLAT"]
                info["on_amp"] = bool(swing == min_amp[ch])
        r64, d64, y64 = r.astype(f64), d.astype(f64), y.astype(f64)
        info["nan_y"], info["nan_r"] = bool(np.isnan(y64).any()), bool(np.isnan(r64).any() or np.isnan(d64).any())
        row = rec[n]
        row[R["OUTCOME"]], row[R["ROWS"]], row[R["CHANNEL"]], row[R["PERIOD"]] = outcome, last - s, ch, P
        row[R["FALL_STEPS"]] = stop - s if outcome == O["FELL"] else -1.0
        row[R["R_MIN"]], row[R["R_MAX"]] = rmin, rmax
        with np.errstate(invalid="ignore", over="ignore"):
            for name, x in (("S_R", r64), ("S_D", d64), ("S_RR", r64 * r64), ("S_DD", d64 * d64), ("S_RD", r64 * d64)):
                row[R[name]] = _ordered_sum(x)
            for k in range(NCH):
                yk = y64[:, k]
                for name, x in (("S_Y", yk), ("S_YY", yk * yk), ("S_YR", yk * r64), ("S_YD", yk * d64)):
                    row[R[name] + k] = _ordered_sum(x)
    return rec, diag


def group_stats_ref(rec, group, G):
    """stats [G, FSTAT SIZE] float64: every group's envs in env order, one float64 operation at a time. group None: all in group 0."""
    rec = np.asarray(rec, f64)
    st = np.zeros((G, S["SIZE"]), f64)
    lo, hi = np.full(G, np.inf), np.full(G, -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(rec.shape[0]):
            g = 0 if group is None else int(group[n])
            if not 0 <= g < G:
                continue
            r = rec[n]
            oc = int(r[R["OUTCOME"]])
            st[g, S["COUNT"] + oc] = st[g, S["COUNT"] + oc] + 1.0
            if oc == O["FELL"]:
                st[g, S["FALL_SUM"]] = st[g, S["FALL_SUM"]] + r[R["FALL_STEPS"]]
            if oc == O["MEASURED"]:
                st[g, S["ROWS"]] = st[g, S["ROWS"]] + r[R["ROWS"]]
                for k in range(NSUMS):
                    st[g, S["SUMS"] + k] = st[g, S["SUMS"] + k] + r[R["S_R"] + k]
                if r[R["R_MIN"]] < lo[g]:
                    lo[g] = r[R["R_MIN"]]
                if r[R["R_MAX"]] > hi[g]:
                    hi[g] = r[R["R_MAX"]]
    some = st[:, S["COUNT"] + O["MEASURED"]] > 0
    st[:, S["R_MIN"]], st[:, S["R_MAX"]] = np.where(some, lo, -1.0), np.where(some, hi, -1.0)
    return st


def frequency_response_ref(sig, sched, min_amp, group, G):
    """(rec, stats) of a given fp32 signal: what kbj_frequency_response's second and third kernel must give."""
    rec, _ = scan_ref(sig, sched, min_amp)
    return rec, group_stats_ref(rec, group, G)


def same_words(got, want):
    """Bit for bit, except that where `want` is NaN `got` only has to be NaN too (float64 arrays)."""
    got, want = np.ascontiguousarray(got, f64), np.ascontiguousarray(want, f64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))


# ---- the host formulas once more ----
def response_ref(rows, sums, k):
    """(gain, lag in rad, coherence) of channel k from `rows` and the 17 sums (FREC order from S_R): the centred products, the 2 x 2 system by
    numpy's solve. nan where host/frequency.lockin says nan."""
    s = np.asarray(sums, f64)
    n = float(rows)
    nan = float("nan")
    if not n > 0:
        return nan, nan, nan
    off = R["S_R"]
    g = lambda name, j=0: s[R[name] - off + j]
    c = lambda sab, sa, sb: sab - sa * sb / n
    M = np.array([[c(g("S_RR"), g("S_R"), g("S_R")), c(g("S_RD"), g("S_R"), g("S_D"))], [c(g("S_RD"), g("S_R"), g("S_D")), c(g("S_DD"), g("S_D"), g("S_D"))]])
    v = np.array([c(g("S_YR", k), g("S_Y", k), g("S_R")), c(g("S_YD", k), g("S_Y", k), g("S_D"))])
    cyy = c(g("S_YY", k), g("S_Y", k), g("S_Y", k))
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    if not det > 0 or not np.isfinite(det):
        return nan, nan, nan
    a, b = np.linalg.solve(M, v)
    return float(np.hypot(a, b)), float(np.arctan2(b, a)), float((a * v[0] + b * v[1]) / cyy) if cyy > 0 else nan


# ---- the synthetic set ----
T_SYN, N_SYN = 333, 130          # T: a multiple of no chunk, room for P = 256, K = 1 behind its 64 lead rows; N: two full wavefronts and a ragged one of 2
NPAT = 26
SEED = 11
MIN_AMP = (0.125, 0.125, 0.25)
EDGE_ROWS = (0, 23, 5, 7, 11)    # where patterns 16 and 17 end the episode, from s: the first and the last scanned row of a P = 8, K = 3 window among them
LEAD_ROWS = (1, 16, 5, 9, 12)    # rows in front of s on which pattern 15 ends an episode: the last and the first of the 16 lead rows among them


class Problem(NamedTuple):
    aux: np.ndarray      # [T + 1, N, AUX SIZE] float32
    sched: np.ndarray    # [N, 4] int32


def problem(T=T_SYN, N=N_SYN, seed=SEED) -> Problem:
    """Env e holds pattern e % NPAT in variant e // NPAT. The driven command word is c + A cos(2 pi (t - s) / P) on every row, the response a
    delayed, scaled copy with a little noise, coupling into the other channels; most envs face along x with an identity quaternion, pattern
    25 carries random attitudes. Every word of an aux row that the entry does not read - and the two command words that are not driven -
    holds noise that changes from row to row."""
    rng = np.random.default_rng(seed)
    aux = rng.uniform(-2.0, 2.0, (T + 1, N, X["SIZE"])).astype(f32)
    aux[:, :, X["DONE"]] = 0.0
    sched = np.zeros((N, 4), np.int64)
    nan = f32("nan")
    t = np.arange(T + 1)
    for n in range(N):
        p, v = n % NPAT, n // NPAT
        s, P, ch, K = 20 + v, 8, (n // 3) % 3, 3
        c, A = 0.25, 0.5
        if p == 0:
            s = -1 - v
        elif p == 1:
            P, s = 4, 10 + v
        elif p == 3:
            P, K = 12, 1
        elif p == 4:
            P, s = 64, 16 + v                                      # v = 0: s == q, the first env that has its lead rows
        elif p == 5:
            P, K, s = 256, 1, 64 + v                               # q = 64: the ring's wrap; the window ends on row 320 + v <= T
        elif p == 6:
            P = 0
        elif p == 7:
            P = 6
        elif p == 8:
            P = 260
        elif p == 9:
            P = -8
        elif p == 10:
            ch = -1
        elif p == 11:
            ch = 3
        elif p == 12:
            K = 0 if v % 2 == 0 else -1 - v
        elif p == 13:
            P, s = 64, 15 - v
        elif p == 14:
            s = T + v if v < 4 else INT32_MAX
        elif p == 15:
            P, s = 64, 40
        elif p == 18:
            P, s = (64, T - 100 - v) if v < 4 else (8, T - 23)     # v = 4: the trajectory cuts the window by one row
        elif p == 19:
            s = T - 24                                             # the window ends with the trajectory: not cut
        elif p == 20:
            P, K = (4, 8, 12, 64, 256)[v], INT32_MAX               # K P needs 64 bits; in 32 it would be -P
            s = 70 + v
        elif p == 21:
            A = 0.0                                                # nobody moved the stick
        elif p == 22:
            P, ch, c = 4, 0, 0.25                                  # r = 0.25 + A {1, 0, -1, 0}: the swing 2 A is MIN_AMP[0] exactly, or one fp32 step of A less
            A = 0.0625 if v % 2 == 0 else 0.0625 - 2.0 ** -20
        elif p == 25:
            P, ch = 12, 2
        sched[n] = (s, P, ch, K)
        se = min(max(s, 0), T)
        Pe = P if P > 0 else 8
        theta = 2.0 * np.pi * (t - se) / Pe
        chan = ch if 0 <= ch <= 2 else 0
        gain, lag = 0.8 - 0.1 * v, 0.3 + 0.2 * v
        vh = rng.uniform(-0.02, 0.02, (T + 1, 3))
        vh[:, chan] += c + gain * A * np.cos(theta - lag)
        vh[:, (chan + 1) % 3] += 0.1 * A * np.sin(theta)
        aux[:, n, X["CMD"] + chan] = (c + A * np.cos(theta)).astype(f32)
        quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (T + 1, 1))
        if p == 25:
            while True:
                q = rng.normal(size=(T + 1, 4)) * 0.15 + np.array([np.cos(0.4 * n), 0.0, 0.0, np.sin(0.4 * n)])
                q /= np.linalg.norm(q, axis=1, keepdims=True)
                if heading64(q.astype(f32))[2].min() >= 0.2:
                    break
            quat = q
        q32 = quat.astype(f32)
        cs, sn, _ = heading64(q32)
        aux[:, n, X["BQUAT"]:X["BQUAT"] + 4] = q32
        aux[:, n, X["QVEL"]] = (cs * vh[:, 0] - sn * vh[:, 1]).astype(f32)
        aux[:, n, X["QVEL"] + 1] = (sn * vh[:, 0] + cs * vh[:, 1]).astype(f32)
        aux[:, n, X["QVEL"] + 5] = vh[:, 2].astype(f32)

        def put(row, col, value):
            if 0 <= row <= T:
                aux[row, n, col] = value
        if p == 15:
            put(s - LEAD_ROWS[v], X["DONE"], 1.0 if v % 2 else -1.0)
        elif p == 16:
            put(s + EDGE_ROWS[v], X["DONE"], -1.0)
        elif p == 17:
            put(s + EDGE_ROWS[v], X["DONE"], 1.0)
        elif p == 23:
            put(s + 3 + v, (X["QVEL"], X["QVEL"] + 1, X["QVEL"] + 5)[v % 3], nan)      # a NaN response sample
        elif p == 24:
            put(s + 2 * v - 1, X["CMD"] + chan, nan)               # a NaN reference sample; v = 0: in the lead rows, it reaches the sums as d alone
        elif p == 25:
            put(s - P // 4 - 1, X["DONE"], -1.0)                   # an episode end in front of the lead rows, and one
            put(s + K * P, X["DONE"], -1.0 if v % 2 else 1.0)      # on the first row behind the window: neither is the window's business
    assert np.abs(sched).max() <= INT32_MAX
    return Problem(aux, sched.astype(np.int32))


def device_like_signal(aux, T):
    """An fp32 signal for the CPU tests: signal_ref rounded to fp32 (stage 2 is an exact function of whichever signal it is given)."""
    return signal_ref(aux, T).astype(f32)


def contents(prob: Problem, min_amp=MIN_AMP) -> dict:
    """What a problem holds, counted from the restatement's own scan (not from the pattern ids)."""
    T = prob.aux.shape[0] - 1
    rec, diag = scan_ref(device_like_signal(prob.aux, T), prob.sched, min_amp)
    oc = rec[:, R["OUTCOME"]]
    c = {name: int((oc == O[name]).sum()) for name in ("NONE", "VOID", "FELL", "MEASURED", "FLAT", "CENSORED")}
    for why in ("period", "channel", "cycles", "lead", "outside", "lead_done"):
        c["void_" + why] = sum(x["void_why"] == why for x in diag)
    for key in ("by_done", "by_T", "nan_y", "nan_r", "on_amp"):
        c[key] = sum(bool(x[key]) for x in diag)
    measured = oc == O["MEASURED"]
    c["periods"] = sorted({int(x) for x in rec[measured, R["PERIOD"]]})
    c["cycles"] = sorted({int(prob.sched[n, 3]) for n in np.flatnonzero(oc >= O["FELL"])})
    for name, want in (("fell", O["FELL"]), ("timeout", O["CENSORED"])):
        rows = [(x["stop_row"], int(prob.sched[n, 1]) * int(prob.sched[n, 3])) for n, x in enumerate(diag) if x["stop_row"] is not None and oc[n] == want]
        c[name + "_first"], c[name + "_last"] = sum(r == 0 for r, _ in rows), sum(r == w - 1 for r, w in rows)
    c["nan_sums"] = int(np.isnan(rec[:, R["S_R"]:]).any(axis=1).sum())
    return c
