"""The command step response, the parts that need no GPU: the layout mirrors, the rule of tests/step_response_ref.py pinned on closed-form
responses and hand-made rows, what its synthetic set contains and that the set tells mutated rules apart (so that
tests/test_gpu_step_response.py means something), the ordered group statistics, the SteppedCommand term through UserTerms.apply_command
against a context that records its calls, the default transitions, the summary and the table."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

from kbot_joystick_amd.spec import compiler, constants, layout as L
from tests import step_response_ref as SR

G_, R, S, O, X = L.SSIG, L.SREC, L.SSTAT, L.SOUT, L.AUX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_layout_mirrors_the_header():
    for table in (L.SSIG, L.SOUT, L.SREC, L.SSTAT):                  # (values against the header: tests/test_abi_mirror.py)
        assert table.get("SIZE", 0) % 4 == 0
    assert L.NSCH == len(constants.STEP_CHANNEL_NAMES) == 3
    assert constants.STEP_CHANNEL_NAMES == ("forward", "sideways", "yaw")
    assert [O[n.upper()] for n in constants.STEP_OUTCOME_NAMES] == list(range(O["COUNT"]))
    assert O["FELL"] == L.POUT["FELL"] and O["CENSORED"] == L.POUT["CENSORED"] and min(O[k] for k in ("FELL", "SETTLED", "UNSETTLED", "CENSORED")) == O["FELL"]
    assert S["COUNT"] + O["COUNT"] == S["SETTLE_SUM"] and S["TRAVEL_ABSMAX"] + L.NSCH <= S["SIZE"] and R["DEV"] + L.NSCH == R["SPARE_TAIL"]
    for a, b in zip(("ACTIVE_N", "RISE_N", "RISE_SUM", "RISE_MAX", "OVER_SUM", "OVER_MAX", "DEV_N", "DEV_SUM", "DEV_MAX", "TRAVEL_SUM"),
                    ("RISE_N", "RISE_SUM", "RISE_MAX", "OVER_SUM", "OVER_MAX", "DEV_N", "DEV_SUM", "DEV_MAX", "TRAVEL_SUM", "TRAVEL_ABSMAX")):
        assert S[a] + L.NSCH == S[b]
    from kbot_joystick_amd.host import binding
    assert ctypes.sizeof(binding.StepCriteria) == 4 * (2 * L.NSCH + 2) + 12 == binding.load_library().kbj_sizeof_step_criteria()
    kbj = open(os.path.join(ROOT, "include", "kbj.h")).read()
    for text in ("float min_step[3];", "float band_abs[3];", "float band_frac;", "float rise_level;", "int32_t smooth_steps, hold_steps, window_steps;",
                 "SETTINGS of the caller, not measured thresholds"):
        assert text in kbj, text
    assert "kbj_step_response" in binding.SIGNATURES and "kbj_sizeof_step_criteria" in binding.SIGNATURES


def _sig(v, cmd0, cmd1, s, done=None):
    """A one-env signal [T, 1, SSIG SIZE] float32: channel values v [T, 3], the command c0 before row s and c1 from it on."""
    T = len(v)
    sig = np.zeros((T, 1, G_["SIZE"]), f32)
    sig[:, 0, :3] = np.asarray(v, f32)
    sig[:s, 0, G_["CMD"]:G_["CMD"] + 3], sig[s:, 0, G_["CMD"]:G_["CMD"] + 3] = cmd0, cmd1
    if done is not None:
        sig[:, 0, G_["DONE"]] = done
    return sig


def test_first_order_response_known_answers():
    """v(t) = c1 + (c0 - c1) exp(-(t - s) / tau) on the forward channel, m = 1, rise level 0.9, band = max(0.05, 0.1 x 1.0) = 0.1.
    p(k) = D (1 - exp(-k / tau)) >= 0.9 D from k = tau ln 10 on: RISE = ceil(tau ln 10), unless the fp32 rounding of v (half an ulp of a value
    below 1: 2^-25, and as much again for the subtraction - the test asks for a margin of 2^-22) reaches across the threshold on the row
    before or on that row; then the answer may be one row off, and the test would say so instead of asserting. |d| = D exp(-k / tau) <= band
    from k = tau ln(D / band) on: SETTLE_STEPS = ceil(tau ln 10) too (band = 0.1 D), and the monotone response never overshoots."""
    T, s, tau, D = 60, 10, 5.0, 1.0
    k = np.arange(T) - s
    v = np.zeros((T, 3))
    v[:, 0] = np.where(k >= 0, D - D * np.exp(-np.maximum(k, 0) / tau), 0.0)
    sig = _sig(v, (0, 0, 0), (D, 0, 0), s)
    crit = SR.Criteria((0.05,) * 3, (0.05,) * 3, 0.1, 0.9, 1, 3, 40)
    rec, _ = SR.scan_ref(sig, [s], crit)
    want = math.ceil(tau * math.log(10.0))
    margin = min(abs(D * math.exp(-(want - 1) / tau) - 0.1 * D), abs(D * math.exp(-want / tau) - 0.1 * D))
    assert want == 12 and margin > 2.0 ** -22, margin                       # no rounding reaches the threshold: the answer is exact
    r = rec[0]
    assert r[R["OUTCOME"]] == O["SETTLED"] and r[R["RISE"]] == want and r[R["OVER"]] == 0.0 and r[R["SETTLE_STEPS"]] == want
    assert r[R["ACTIVE"]] == 1 and r[R["RISE"] + 1] == r[R["OVER"] + 1] == r[R["DEV"]] == -1 and r[R["DEV"] + 1] == r[R["DEV"] + 2] == 0.0
    assert r[R["FALL_STEPS"]] == -1 and r[R["SPARE"]] == 0 and (r[R["SPARE_TAIL"]:] == 0).all()
    # travel: the raw rows s .. s + want + hold - 1, summed in float64 and rounded once
    assert r[R["TRAVEL_X"]] == f32(sig[s:s + want + 3, 0, 0].astype(np.float64).sum()) and r[R["TRAVEL_Y"]] == 0 and r[R["TRAVEL_YAW"]] == 0
    # the same response downwards (a stop from 1 m/s): the same figures, and the travel is the stopping distance in (m/s) x rows
    down = np.zeros((T, 3))
    down[:, 0] = D - v[:, 0]
    sig2 = _sig(down, (D, 0, 0), (0, 0, 0), s)
    r2 = SR.scan_ref(sig2, [s], crit)[0][0]
    assert r2[R["OUTCOME"]] == O["SETTLED"] and r2[R["RISE"]] == want and r2[R["OVER"]] == 0.0 and r2[R["SETTLE_STEPS"]] == want
    closed = sum(math.exp(-j / tau) for j in range(want + 3))
    assert abs(r2[R["TRAVEL_X"]] - closed) < 1e-5
    # a window one row too short for the hold run: UNSETTLED; the same with the trajectory cut there: CENSORED
    short = crit._replace(window=want + 2)
    assert SR.scan_ref(sig, [s], short)[0][0, R["OUTCOME"]] == O["UNSETTLED"]
    assert SR.scan_ref(sig[:s + want + 2], [s], crit)[0][0, R["OUTCOME"]] == O["CENSORED"]
    # smoothing over m = 4 rows delays the rise (the mean of the last four rows lags the last one)
    assert SR.scan_ref(sig, [s], crit._replace(smooth=4))[0][0, R["RISE"]] > want


def test_underdamped_response_overshoot():
    """The unit step response of a second-order system, v(k) = D (1 - exp(-a k) (cos(w k) + (a / w) sin(w k))), has its first peak at w k = pi
    with the overshoot D exp(-a pi / w). With w = pi / 8 the peak falls on row s + 8 exactly; OVER is the fp32 sample there minus c1: within
    a few ulp of 1 of the closed form (the test allows 4 x 2^-23)."""
    T, s, D, a, w = 70, 6, 1.0, 0.15, math.pi / 8
    k = np.maximum(np.arange(T) - s, 0)
    v = np.zeros((T, 3))
    v[:, 2] = np.where(np.arange(T) >= s, -D * (1 - np.exp(-a * k) * (np.cos(w * k) + a / w * np.sin(w * k))), 0.0)      # a step to the right: downwards
    sig = _sig(v, (0, 0, 0), (0, 0, -D), s)
    crit = SR.Criteria((0.05,) * 3, (0.05,) * 3, 0.05, 0.9, 1, 5, 60)
    r = SR.scan_ref(sig, [s], crit)[0][0]
    over = D * math.exp(-a * math.pi / w)
    assert r[R["ACTIVE"]] == 4 and abs(r[R["OVER"] + 2] - over) <= 4 * 2.0 ** -23 and over > 0.3
    assert r[R["OUTCOME"]] == O["SETTLED"] and r[R["RISE"] + 2] < 8 and r[R["SETTLE_STEPS"]] > 8      # it settles only after the first peak
    assert r[R["DEV"]] == 0 and r[R["OVER"]] == -1


def test_hand_made_rows():
    """T = 12, hold = 2, window = 6, m = 2, the step on row 4 from 0 to 1 m/s forward; band 0.25, threshold 0.5."""
    crit = SR.Criteria((0.05,) * 3, (0.25,) * 3, 0.1, 0.5, 2, 2, 6)
    v = np.zeros((12, 3))
    v[4:, 0] = (0.2, 0.6, 1.4, 1.0, 1.0, 1.0, 1.0, 1.0)          # smoothed from row 4 (over the rows from s - hold = 2 on): 0.1, 0.4, 1.0, 1.2, 1.0, 1.0
    v[6, 1] = 0.3                                                # sideways, not commanded: smoothed 0.15 on rows 6 and 7
    base = _sig(v, (0, 0, 0), (1, 0, 0), 4)
    r = SR.scan_ref(base, [4], crit)[0][0]
    # rise: S = 1.0 >= 0.5 on row 6 (k = 2); over: 1.2 - 1 on row 7; within (|d| <= 0.25) on rows 6, 7 -> settled, first row of the run 6
    assert (r[R["OUTCOME"]], r[R["SETTLE_STEPS"]], r[R["RISE"]]) == (O["SETTLED"], 2, 2)
    assert r[R["OVER"]] == f32(f32(1.2) - f32(1.0)) and r[R["DEV"] + 1] == f32(0.15) and r[R["DEV"] + 2] == 0
    assert r[R["TRAVEL_X"]] == f32(np.float64(f32(0.2)) + np.float64(f32(0.6)) + np.float64(f32(1.4)) + 1.0) and r[R["TRAVEL_Y"]] == f32(0.3)
    cases = []
    fell = base.copy(); fell[5, 0, G_["DONE"]] = -1
    cases.append((fell, 4, O["FELL"], dict(FALL_STEPS=1)))
    out = base.copy(); out[6, 0, G_["DONE"]] = 1
    cases.append((out, 4, O["CENSORED"], {}))
    again = base.copy(); again[5:, 0, G_["CMD"] + 2] = 0.5
    cases.append((again, 4, O["CENSORED"], {}))
    late = base.copy(); late[8, 0, G_["DONE"]] = -1                # behind the deciding row: not seen
    cases.append((late, 4, O["SETTLED"], dict(SETTLE_STEPS=2)))
    for sig, s, oc, fields in cases:
        x = SR.scan_ref(sig, [s], crit)[0][0]
        assert x[R["OUTCOME"]] == oc and all(x[R[k]] == val for k, val in fields.items()), (oc, x)
    # VOID, every way
    pre_done = base.copy(); pre_done[2, 0, G_["DONE"]] = 1
    pre_cmd = base.copy(); pre_cmd[2, 0, G_["CMD"] + 1] = 0.5
    off = base.copy(); off[3, 0, 2] = 0.6                          # smoothed yaw rate 0.3 > 0.25 on the row in front of the step
    nan = base.copy(); nan[2, 0, 0] = np.nan
    small = _sig(v, (0, 0, 0), (0.04, 0, 0), 4)
    for sig, s in ((pre_done, 4), (pre_cmd, 4), (off, 4), (nan, 4), (small, 4), (base, 1), (base, 12), (base, 2 ** 31 - 1)):
        x = SR.scan_ref(sig, [s], crit)[0][0]
        assert x[R["OUTCOME"]] == O["VOID"] and (x[1:R["SPARE"]] == -1).all() and (x[R["RISE"]:R["SPARE_TAIL"]] == -1).all() and x[R["SPARE"]] == 0, x
    x = SR.scan_ref(base, [-3], crit)[0][0]
    assert x[R["OUTCOME"]] == O["NONE"] and (x[1:R["SPARE"]] == -1).all()
    # a NaN in the channel that did not move breaks the run for m rows and is no deviation
    quiet = base.copy(); quiet[6, 0, 2] = np.nan
    x = SR.scan_ref(quiet, [4], crit)[0][0]
    assert (x[R["OUTCOME"]], x[R["SETTLE_STEPS"]], x[R["DEV"] + 2]) == (O["SETTLED"], 4, 0) and np.isnan(x[R["TRAVEL_YAW"]])


COMBOS = [(m, hold) for m in (1, 3, 32) for hold in (1, 4)]


@pytest.mark.parametrize("m,hold", COMBOS)
def test_synthetic_set_coverage(m, hold):
    prob, crit = SR.problem(hold), SR.criteria(m, hold)
    c = SR.contents(prob, crit)
    print(m, hold, c)
    for name in ("NONE", "VOID", "FELL", "SETTLED", "UNSETTLED", "CENSORED"):
        assert c[name] >= 5, (name, c)
    for k in range(L.NSCH):
        assert c[f"active_{k}"] >= 10 and c[f"inactive_{k}"] >= 10, (k, c)
    for key in ("void_outside", "void_pre_done", "void_inactive", "void_off_command", "nan_pre", "nan_scan", "nan_inactive", "by_done", "by_cmd", "by_T", "never_rose"):
        assert c[key] >= 3, (key, c)
    if m == 1:
        assert c["on_band"] >= 3 and c["on_thr"] >= 3 and c["done_after_settle"] >= 3 and c["overshoot"] >= 3, c
    if hold > 1:
        assert c["void_pre_cmd"] >= 3, c
    s = prob.sched.astype(np.int64)
    T = SR.T_SYN
    assert prob.aux.shape == (T + 1, SR.N_SYN, X["SIZE"]) and SR.N_SYN == 130 and T == 75
    for value in (-1, 0, hold - 1, T - 1, T, SR.INT32_MAX):
        assert (s == value).any(), value
    assert ((s < T) & (s + SR.WINDOW > T) & (s >= hold)).sum() >= 3
    q = prob.aux[:T, :, X["BQUAT"]:X["BQUAT"] + 4]
    h = SR.heading64(q)[2]
    assert (h == 0).any() and (h[h > 0] >= 0.2).all() and ((h > 0) & (np.abs(q[..., 0]) < 0.99)).any()      # the degenerate heading, and real attitudes
    again = SR.problem(hold)
    assert np.array_equal(prob.aux, again.aux, equal_nan=True) and np.array_equal(prob.sched, again.sched)     # deterministic
    g = SR.groups(SR.N_SYN, 3)
    assert g[1] == 3 and g[2] == -1 and set(g.tolist()) == {-1, 0, 1, 2, 3}


def test_the_set_tells_mutated_rules_apart():
    """Each mutant breaks one clause (check order of FELL against CENSORED and against the settle test, the run reset, the start of the
    smoothing window at s - hold, the censor rule s + window > T, VOID on the rows in front of the step). For each there is a (smooth, hold)
    of the GPU test under which the synthetic set gives it another record than the rule."""
    told = {mu: [] for mu in SR.MUTANTS}
    for m, hold in COMBOS:
        prob, crit = SR.problem(hold), SR.criteria(m, hold)
        sig = SR.device_like_signal(prob.aux, SR.T_SYN)
        rec, _ = SR.scan_ref(sig, prob.sched, crit)
        for mu in SR.MUTANTS:
            other, _ = SR.scan_ref(sig, prob.sched, crit, mu)
            if (rec.view(np.uint32) != other.view(np.uint32)).any():
                told[mu].append((m, hold))
    print(told)
    assert all(told.values()), told
    assert (1, 4) in told["run_not_reset"] and (3, 1) in told["smooth_from_zero"] and len(told["censor_at_equal"]) == len(COMBOS)


def test_group_statistics_are_ordered_and_skip_strangers():
    prob, crit = SR.problem(4), SR.criteria(3, 4)
    sig = SR.device_like_signal(prob.aux, SR.T_SYN)
    rec, _ = SR.scan_ref(sig, prob.sched, crit)
    N = SR.N_SYN
    for G in (1, 3, 256):
        st = SR.group_stats_ref(rec, SR.groups(N, G), G)
        assert st[:, S["COUNT"]:S["COUNT"] + O["COUNT"]].sum() == N - 2                        # envs 1 and 2 are in no group
        assert (st[:, S["TRAVEL_ABSMAX"] + L.NSCH:] == 0).all()
    one = SR.group_stats_ref(rec, None, 1)[0]
    assert one[S["COUNT"]:S["COUNT"] + O["COUNT"]].sum() == N
    oc, act = rec[:, R["OUTCOME"]], rec[:, R["ACTIVE"]].astype(int)
    valid, settled = oc >= O["FELL"], oc == O["SETTLED"]
    for k in range(L.NSCH):
        on = valid & ((act >> k & 1) == 1)
        assert one[S["ACTIVE_N"] + k] == on.sum() and one[S["DEV_N"] + k] == (valid & ~on).sum()
        assert one[S["RISE_N"] + k] == (on & (rec[:, R["RISE"] + k] >= 0)).sum()
        seq = np.float64(0)
        for x in rec[on, R["OVER"] + k]:
            seq = seq + np.float64(x)
        assert one[S["OVER_SUM"] + k] == seq and one[S["OVER_MAX"] + k] == rec[on, R["OVER"] + k].max()
    assert one[S["SETTLE_SUM"]] == rec[settled, R["SETTLE_STEPS"]].astype(np.float64).sum() and one[S["SETTLE_MAX"]] == rec[settled, R["SETTLE_STEPS"]].max()
    assert np.isnan(one[S["TRAVEL_SUM"]]) and one[S["TRAVEL_ABSMAX"]] >= 0                     # a NaN travel reaches the sum and never a maximum
    empty = SR.group_stats_ref(rec[:0], None, 2)
    assert (empty[:, [S["SETTLE_MAX"], S["FALL_MAX"], S["RISE_MAX"], S["OVER_MAX"] + 1, S["DEV_MAX"] + 2, S["TRAVEL_ABSMAX"]]] == -1).all() and empty[:, :S["SETTLE_MAX"]].sum() == 0


class _Recorder:
    """Stands in for a Context: keeps what apply_command sends to kbj_env_set_command and writes it into the aux row, as the kernel does."""
    def __init__(self):
        self.calls = []

    def env_set_command(self, mask, cmd, actor, critic, aux):
        assert mask is None
        self.calls.append(cmd.clone())
        aux[:, X["CMD"]:X["CMD"] + L.NCMD] = cmd


class _Rows:
    def __init__(self, T, N):
        self.actor_obs, self.critic_obs, self.aux = torch.zeros(T + 1, N, L.LD_ACTOR), torch.zeros(T + 1, N, L.LD_CRITIC), torch.zeros(T + 1, N, X["SIZE"])


def test_stepped_command_schedule():
    """Rows 0 .. 6 of three envs, the step on row 3. Env 1's episode ends in step 1 (fresh on row 2), env 2's in step 4 (fresh on row 5): the
    kernel's reset has put the context's fixed command (here 9s) into their rows, and the term writes the scheduled command again."""
    from kbot_joystick_amd.host.step import SteppedCommand
    from kbot_joystick_amd.host.user_terms import UserTerms
    T, N = 6, 3
    tr, ctx = _Rows(T, N), _Recorder()
    tr.aux[:, :, X["BQUAT"]] = 1.0
    tr.aux[1, 1, X["DONE"]], tr.aux[4, 2, X["DONE"]] = -1.0, 1.0
    tr.aux[2, 1, X["CMD"]:X["CMD"] + L.NCMD] = 9.0
    tr.aux[5, 2, X["CMD"]:X["CMD"] + L.NCMD] = 9.0
    t0, t1 = torch.zeros(N, L.NCMD), torch.zeros(N, L.NCMD)
    t0[:, 0], t1[:, 0], t1[:, 2] = torch.tensor([0.0, 0.5, 1.0]), torch.tensor([1.0, -0.5, 0.0]), 0.25
    terms = UserTerms(command=SteppedCommand(t0, t1, 3))
    terms.bind(5, 0, torch.device("cpu"), compiler.load_model("kbot-headless"), L.NOBS_ACTOR, L.NOBS_CRITIC)
    for row in range(T + 1):
        terms.run_hooks(ctx, tr, row, 100 + row, [terms.apply_command])
    assert len(ctx.calls) == T + 1
    for row, cmd in enumerate(ctx.calls):
        assert torch.equal(cmd, t0 if row < 3 else t1), row
        assert torch.equal(tr.aux[row, :, X["CMD"]:X["CMD"] + L.NCMD], t0 if row < 3 else t1)


def test_default_step_grid():
    from kbot_joystick_amd.host.step import default_step_grid
    k = L.default_config()
    grid = default_step_grid(k)
    z = (0.0,) * 16
    one = lambda i, v: tuple(float(np.float32(v)) if j == i else 0.0 for j in range(16))
    near = lambda a, b: np.allclose(a, b, atol=1e-6)
    want = [(z, one(0, k.vx_hi)), (one(0, k.vx_hi), z), (z, one(0, k.vx_lo)), (z, one(1, k.vy_hi)), (one(1, k.vy_hi), z), (z, one(2, k.wz_hi)), (one(2, k.wz_hi), z),
            (one(0, 0.5 * k.vx_hi), one(0, k.vx_hi)), (one(0, k.vx_hi), one(0, k.vx_lo)), (one(2, k.wz_hi), one(2, k.wz_lo))]
    assert len(grid) == 10 and all(len(a) == len(b) == 16 for a, b in grid)
    assert all(near(a, wa) and near(b, wb) for (a, b), (wa, wb) in zip(grid, want))
    assert k.vx_hi > 0 > k.vx_lo and k.vy_hi > 0 and k.wz_hi > 0 > k.wz_lo          # forward, backward, left, turn left, turn right are what they are called


def test_case_summary_and_table():
    from kbot_joystick_amd.host.step import case_summary, format_step_table
    vec = np.zeros(S["SIZE"])
    vec[S["COUNT"] + O["VOID"]], vec[S["COUNT"] + O["FELL"]], vec[S["COUNT"] + O["SETTLED"]], vec[S["COUNT"] + O["CENSORED"]] = 1, 1, 2, 1
    vec[S["SETTLE_SUM"]], vec[S["SETTLE_SUMSQ"]], vec[S["SETTLE_MAX"]] = 60, 2000, 40
    vec[S["FALL_SUM"]], vec[S["FALL_MAX"]] = 15, 15
    vec[S["ACTIVE_N"]], vec[S["RISE_N"]], vec[S["RISE_SUM"]], vec[S["RISE_MAX"]], vec[S["OVER_SUM"]], vec[S["OVER_MAX"]] = 4, 3, 45, 20, 0.8, 0.4
    for k in (1, 2):
        vec[S["DEV_N"] + k], vec[S["DEV_SUM"] + k], vec[S["DEV_MAX"] + k] = 4, 0.4 * k, 0.2 * k
        vec[S["RISE_MAX"] + k] = vec[S["OVER_MAX"] + k] = -1
    vec[S["DEV_MAX"]] = -1
    vec[S["TRAVEL_SUM"]], vec[S["TRAVEL_ABSMAX"]], vec[S["TRAVEL_SUM"] + 2], vec[S["TRAVEL_ABSMAX"] + 2] = 50, 30, -5, 4
    x = case_summary(vec, 0.02)
    assert (x["valid"], x["void"], x["fell_frac"], x["settled_frac"], x["unsettled_frac"], x["censored_frac"]) == (4, 1, 0.25, 0.5, 0.0, 0.25)
    assert x["settle_s_mean"] == pytest.approx(0.6) and x["settle_s_max"] == pytest.approx(0.8) and x["fall_s_mean"] == pytest.approx(0.3)
    assert x["forward_active"] == 4 and x["forward_risen_frac"] == 0.75 and x["forward_rise_s_mean"] == pytest.approx(0.3) and x["forward_rise_s_max"] == pytest.approx(0.4)
    assert x["forward_overshoot_mean"] == pytest.approx(0.2) and x["forward_overshoot_max"] == 0.4 and math.isnan(x["forward_coupling_mean"]) and math.isnan(x["forward_coupling_max"])
    assert x["sideways_active"] == 0 and math.isnan(x["sideways_rise_s_mean"]) and math.isnan(x["sideways_overshoot_max"]) and x["sideways_coupling_mean"] == pytest.approx(0.1)
    assert x["yaw_coupling_max"] == 0.4 and x["forward_travel_mean"] == pytest.approx(0.5) and x["forward_travel_absmax"] == pytest.approx(0.6)      # metres
    assert x["yaw_travel_mean"] == pytest.approx(-0.05) and x["sideways_travel_mean"] == 0.0
    none = np.zeros(S["SIZE"])
    for name in ("SETTLE_MAX", "FALL_MAX"):
        none[S[name]] = -1
    for name in ("RISE_MAX", "OVER_MAX", "DEV_MAX", "TRAVEL_ABSMAX"):
        none[S[name]:S[name] + 3] = -1
    empty = case_summary(none, 0.02)
    assert empty["valid"] == 0 and all(math.isnan(v) for k, v in empty.items() if k not in ("valid", "void") and not k.endswith("_active"))
    settings = dict(step_at=3.0, window=4.0, hold=0.5, smooth=0.5, rise_level=0.9, band_frac=0.1, band_abs=(0.15, 0.15, 0.25), min_step=(0.05, 0.05, 0.05), repeats=4)
    z = (0.0,) * 16
    fwd = (1.2,) + (0.0,) * 15
    text = format_step_table([dict(from_command=z, to_command=fwd, **settings, **x), dict(from_command=fwd, to_command=z, **settings, **empty)])
    lines = text.splitlines()
    assert len(lines) == 4 and "settings, not measured thresholds" in lines[0] and "rise level 0.9" in lines[0] and "yaw: band>=0.25 step>=0.05" in lines[0]
    assert lines[2].startswith("(zero) -> xvel=+1.20") and lines[2].split()[3:7] == ["4", "1", "0.250", "0.500"] and lines[3].startswith("xvel=+1.20 -> (zero)")
    assert " - " in lines[3] + " " and "nan" not in text
    assert format_step_table([]).count("\n") == 0


def test_sweep_refuses_what_the_kernel_cannot_take():
    from kbot_joystick_amd.host.step import step_sweep
    task = types.SimpleNamespace(config=types.SimpleNamespace(ctrl_dt=0.02), kcfg=L.default_config())
    with pytest.raises(ValueError, match=r"smooth = 0.7 s is 35 rows .* at most 32 rows"):
        step_sweep(task, smooth=0.7)
    with pytest.raises(ValueError, match="at most 256"):
        step_sweep(task, transitions=[((0.0,), (0.5,))] * 257)
    with pytest.raises(ValueError, match="room for the hold rows"):
        step_sweep(task, step_at=0.2, hold=0.5)
    with pytest.raises(ValueError, match="at least one transition"):
        step_sweep(task, transitions=[])
    with pytest.raises(ValueError, match="17 components"):
        step_sweep(task, transitions=[((0.0,) * 17, (0.5,))])
