"""Host restatement of kbj_episode_stats (include/kbj.h): a float32 loop per env for the accumulators, math.fsum / float64 for the
reductions over the finished episodes. Shared by tests/test_episode_stats_host.py and tests/test_gpu_episode_stats.py."""
import math

import numpy as np

from kbot_joystick_amd.spec import layout as L

E, A, X = L.EPST, L.EACC, L.AUX
COUNT_SLOTS = ("EPISODES", "FAIL_HEIGHT", "FAIL_OTHER", "TRUNCATED")
EXACT_SLOTS = COUNT_SLOTS + ("RETURN_MIN", "RETURN_MAX", "LENGTH_MAX")
SUM_SLOTS = ("RETURN_SUM", "RETURN_SUMSQ", "LENGTH_SUM", "FAIL_LENGTH_SUM")


def episode_stats_ref(acc, reward, aux, comps, unhealthy_z):
    """acc [N, 16] float32 (updated IN PLACE), reward [T, N], aux [T(+1), N, 72], comps [T, N, 12] or None.
    Returns (stats [EPST SIZE] float64, mags): mags[slot] = sum of |x_i| over what the slot adds up (the scale of its rounding bound)."""
    T, N = reward.shape
    f32 = np.float32
    uz = f32(unhealthy_z)
    eps = []            # (return, length, kind, terms[12]) of every finished episode, fp32 values
    for n in range(N):
        row = acc[n]
        for t in range(T):
            row[A["RETURN"]] = f32(row[A["RETURN"]] + f32(reward[t, n]))
            row[A["LENGTH"]] = f32(row[A["LENGTH"]] + f32(1.0))
            if comps is not None:
                for k in range(L.NREW):
                    row[A["TERM"] + k] = f32(row[A["TERM"] + k] + f32(comps[t, n, k]))
            d = aux[t, n, X["DONE"]]
            if d != 0:
                if d < 0:
                    h = f32(f32(aux[t, n, X["BASEZ"]]) - min(f32(aux[t, n, X["LFZ"]]), f32(aux[t, n, X["RFZ"]])))
                    kind = "FAIL_HEIGHT" if h < uz else "FAIL_OTHER"
                else:
                    kind = "TRUNCATED"
                eps.append((row[A["RETURN"]], row[A["LENGTH"]], kind, row[A["TERM"]:A["TERM"] + L.NREW].copy()))
                row[:A["TERM"] + L.NREW] = 0
    st = np.zeros(E["SIZE"], np.float64)
    st[E["RETURN_MIN"]], st[E["RETURN_MAX"]] = np.inf, -np.inf
    mags = {}
    ret = [float(e[0]) for e in eps]
    ln = [float(e[1]) for e in eps]
    fl = [float(e[1]) for e in eps if e[2] != "TRUNCATED"]
    st[E["EPISODES"]] = len(eps)
    for kind in ("FAIL_HEIGHT", "FAIL_OTHER", "TRUNCATED"):
        st[E[kind]] = sum(1 for e in eps if e[2] == kind)
    for slot, xs in (("RETURN_SUM", ret), ("RETURN_SUMSQ", [r * r for r in ret]), ("LENGTH_SUM", ln), ("FAIL_LENGTH_SUM", fl)):
        st[E[slot]] = math.fsum(xs)
        mags[slot] = math.fsum(abs(x) for x in xs)
    if eps:
        st[E["RETURN_MIN"]], st[E["RETURN_MAX"]], st[E["LENGTH_MAX"]] = min(ret), max(ret), max(ln)
    for k in range(L.NREW):
        xs = [float(e[3][k]) for e in eps]
        st[E["TERM_SUM"] + k] = math.fsum(xs)
        mags[f"TERM_SUM{k}"] = math.fsum(abs(x) for x in xs)
    return st, mags


def assert_stats_match(got, want, mags, rel=1e-9):
    """Counts, min, max and the longest episode exactly; every double sum within rel * sum |x_i| of the fsum value."""
    got = np.asarray(got, np.float64)
    for slot in EXACT_SLOTS:
        assert got[E[slot]] == want[E[slot]], (slot, got[E[slot]], want[E[slot]])
    for slot in SUM_SLOTS:
        assert abs(got[E[slot]] - want[E[slot]]) <= rel * mags[slot], (slot, got[E[slot]], want[E[slot]], mags[slot])
    for k in range(L.NREW):
        i = E["TERM_SUM"] + k
        assert abs(got[i] - want[i]) <= rel * mags[f"TERM_SUM{k}"], (f"TERM_SUM[{k}]", got[i], want[i])
    used = {E[s] for s in EXACT_SLOTS + SUM_SLOTS} | {E["TERM_SUM"] + k for k in range(L.NREW)}
    for i in range(E["SIZE"]):
        if i not in used:
            assert got[i] == 0.0, ("spare slot", i, got[i])
