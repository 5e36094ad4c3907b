"""Scripted pushes and push recovery, the parts that need no GPU: the layout mirrors, the recovery rule pinned on a hand-computed case, what
the synthetic problems of tests/push_ref.py contain (so that tests/test_gpu_push.py means something), the ordered group sums, the
PushRequest checks, ScriptedPush's schedule through UserTerms.apply_events against a context that records its calls, the heading-frame
rotation against a float64 formula, and the table."""
import math
import os

import numpy as np
import pytest
import torch

from kbot_joystick_amd.spec import compiler, constants, layout as L
from tests import push_ref as PR

P, S, O, R, X = L.PREC, L.PSTAT, L.POUT, L.TERR, L.AUX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "kbj_model.h")).read()
    assert L.PUSH_NEVER == 2.0 ** 24                                                        # (values against the header: tests/test_abi_mirror.py)
    assert np.float32(L.PUSH_NEVER) - np.float32(1) == L.PUSH_NEVER - 1                     # exactly countable in fp32
    assert [O[n.upper()] for n in constants.PUSH_OUTCOME_NAMES] == list(range(O["COUNT"]))
    assert P["PEAK_LIN"] + L.NPEAK == P["PEAK_ROW"] and S["COUNT"] + O["COUNT"] == S["REC_SUM"] and S["PEAK_MAX"] + L.NPEAK <= S["SIZE"]
    for name in ("KBJ_ES_PUSH_REM", "KBJ_ES_PUSH_NXT"):                                       # counted in control steps, and said so
        line = next(l for l in hdr.splitlines() if name + " " in l and "=" in l)
        assert "control steps" in line and "substeps" not in line, line
    from kbot_joystick_amd.host import binding
    import ctypes
    assert ctypes.sizeof(binding.PushCriteria) == 4 * L.NTERR + 8
    kbj = open(os.path.join(ROOT, "include", "kbj.h")).read()
    assert "float tol[KBJ_NTERR];" in kbj and "int32_t hold_steps, window_steps;" in kbj


def test_hand_computed_scan():
    """T = 10, hold = 2, window = 4, five envs with the push on row 3 for d = 1 (rows 3; post rows from 4), tolerances (1, 1, 1, inf, 1)."""
    T, N = 10, 5
    err = np.zeros((T, N, R["SIZE"]), np.float32)
    done = np.zeros((T, N), np.float32)
    sched = np.tile(np.array([[3, 1]], np.int32), (N, 1))
    tol = (1.0, 1.0, 1.0, float("inf"), 1.0)
    err[:, :, R["HEIGHT"]] = 50.0                                  # ignored by the inf tolerance, but a peak
    err[3, 0, R["TILT"]], err[4, 0, R["TILT"]], err[5, 0, R["LIN"]] = 3.0, 7.0, 2.0      # env 0: out on rows 3, 4, 5; within on 6, 7 -> recovered, first row of the run 6
    err[2, 1, R["YAW"]] = 2.0                                      # env 1: a hold row is out -> VOID
    err[3:, 2, R["ARM"]] = 2.0                                     # env 2: out for good -> rows 3..7 seen, UNRECOVERED
    err[4, 2, R["TILT"]], err[6, 2, R["TILT"]] = 0.5, 0.5          #        the tilt peak is reached FIRST on row 4
    done[5, 3] = -1.0                                              # env 3: falls on row 5
    err[5, 3, R["LIN"]] = np.nan                                   #        a NaN is no peak
    done[4, 4] = 1.0                                               # env 4: a time-out on row 4
    rec, _ = PR.recovery_ref(err, done, sched, tol, 2, 4)
    row = lambda oc, rs, fs, pl, py, pt, ph, pr: [oc, rs, fs, pl, py, pt, ph, pr]
    assert rec[0].tolist() == row(O["RECOVERED"], 2, -1, 2, 0, 7, 50, 4)
    assert rec[1].tolist() == row(O["VOID"], -1, -1, -1, -1, -1, -1, -1)
    assert rec[2].tolist() == row(O["UNRECOVERED"], -1, -1, 0, 0, 0.5, 50, 4)
    assert rec[3].tolist() == row(O["FELL"], -1, 2, 0, 0, 0, 50, 3)
    assert rec[4].tolist() == row(O["CENSORED"], -1, -1, 0, 0, 0, 50, 3)
    # the same schedule, the trajectory one row shorter than the window of env 2 (3 + 1 + 4 = 8 > 7): CENSORED instead of UNRECOVERED
    rec7, _ = PR.recovery_ref(err[:7], done[:7], sched, tol, 2, 4)
    assert rec7[2, P["OUTCOME"]] == O["CENSORED"] and rec7[0, P["OUTCOME"]] == O["CENSORED"]     # env 0's run is one row long when the rows end
    st = PR.group_stats_ref(rec, np.array([0, 0, 1, 1, 0], np.int32), 2)
    want0 = np.zeros(S["SIZE"]); want0[S["COUNT"] + O["RECOVERED"]] = want0[S["COUNT"] + O["VOID"]] = want0[S["COUNT"] + O["CENSORED"]] = 1
    want0[S["REC_SUM"]], want0[S["REC_SUMSQ"]], want0[S["REC_MAX"]], want0[S["FALL_MAX"]] = 2, 4, 2, -1
    want0[S["PEAK_SUM"]:S["PEAK_SUM"] + 4], want0[S["PEAK_MAX"]:S["PEAK_MAX"] + 4] = (2, 0, 7, 100), (2, 0, 7, 50)
    assert st[0].tolist() == want0.tolist()
    assert (st[1, S["COUNT"] + O["FELL"]], st[1, S["COUNT"] + O["UNRECOVERED"]], st[1, S["FALL_SUM"]], st[1, S["FALL_SUMSQ"]], st[1, S["REC_MAX"]]) == (1, 1, 2, 4, -1)


@pytest.mark.parametrize("T,N", [s for s in PR.SHAPES + PR.CHUNK_SHAPES if PR.FULL(*s)])
def test_problems_hold_every_case_three_times(T, N):
    prob = PR.problems(T, N)
    assert sum(math.isinf(t) for t in prob.tol) == 1 and prob.hold >= 2 and prob.window > prob.hold
    assert np.isnan(prob.err[:, :, :L.NTERR]).any() and np.isnan(prob.err[:, :, R["HEIGHT"]]).any()     # a NaN in the ignored column too
    c = PR.contents(prob)
    print(T, N, c)
    assert all(v >= 3 for v in c.values()), c
    again = PR.problems(T, N)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(prob[:3], again[:3]))     # deterministic
    g = PR.groups(N, 5)
    assert g[1] == 5 and ((g[np.arange(N) != 1] >= 0) & (g[np.arange(N) != 1] < 5)).all() and len(set(g.tolist())) == 6


def test_group_sums_are_ordered_and_skip_strangers():
    prob = PR.problems(40, 64)
    rec, _ = PR.recovery_ref(prob.err, prob.done, prob.sched, prob.tol, prob.hold, prob.window)
    for G in (1, 5, 64):
        st = PR.group_stats_ref(rec, PR.groups(64, G), G)
        assert st[:, S["COUNT"]:S["COUNT"] + O["COUNT"]].sum() == 63                       # env 1 is in no group
        assert (st[:, S["PEAK_MAX"] + L.NPEAK:] == 0).all()
    one = PR.group_stats_ref(rec, None, 1)[0]
    assert one[S["COUNT"]:S["COUNT"] + O["COUNT"]].sum() == 64
    scanned = rec[:, P["OUTCOME"]] >= O["FELL"]
    seq = np.float64(0)
    for x in rec[scanned, P["PEAK_TILT"]]:
        seq = seq + np.float64(x)
    assert one[S["PEAK_SUM"] + 2] == seq and one[S["PEAK_MAX"] + 2] == rec[scanned, P["PEAK_TILT"]].max()


def test_push_request_checks_name_the_term_and_the_field():
    from kbot_joystick_amd.host.binding import KbjError
    from kbot_joystick_amd.host.traj_view import PushRequest
    from kbot_joystick_amd.host.user_terms import check_push_request
    n = 4
    good = dict(mask=torch.tensor([True, False, True, False]), wrench=torch.zeros(n, 6), steps=torch.tensor([5.0, float("nan"), 0.0, -3.0]))
    out = check_push_request("shove", PushRequest(**good), n)                      # rows outside the mask are not read
    assert out.next is None and out.steps.dtype == torch.float32
    out = check_push_request("shove", PushRequest(**good, next=torch.full((n,), L.PUSH_NEVER)), n)
    assert out.next[0] == L.PUSH_NEVER
    cases = [(dict(good, wrench=torch.zeros(n, 3)), r"'shove' returned wrench of shape \(4, 3\), expected \(4, 6\)"),
             (dict(good, steps=torch.zeros(n, 1)), r"steps of shape \(4, 1\), expected \(4,\)"),
             (dict(good, mask=torch.ones(n)), r"mask of dtype torch.float32, expected torch.bool"),
             (dict(good, mask=None), r"mask of shape NoneType"),
             (dict(good, wrench=torch.full((n, 6), float("inf"))), r"non-finite values in wrench"),
             (dict(good, steps=torch.tensor([2.5, 0, 0, 0])), r"steps that are not whole numbers in \[0, 16777216\]"),
             (dict(good, steps=torch.tensor([0, 0, -1.0, 0])), r"steps that are not whole numbers"),
             (dict(good, steps=torch.tensor([2.0 ** 25, 0, 0, 0])), r"steps that are not whole numbers"),
             (dict(good, steps=torch.tensor([float("nan"), 0, 0, 0])), r"steps that are not whole numbers"),
             (dict(good, next=torch.tensor([0.5, 0, 0, 0])), r"next that are not whole numbers"),
             (dict(good, next=torch.zeros(n + 1)), r"next of shape \(5,\), expected \(4,\)")]
    for kw, msg in cases:
        with pytest.raises(KbjError, match=msg):
            check_push_request("shove", PushRequest(**kw), n)
    with pytest.raises(KbjError, match="returned tuple as its push"):
        check_push_request("shove", (good["mask"], good["wrench"], good["steps"]), n)


def _yaw_rotate64(q, v):
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    yaw = np.arctan2(2 * (q[:, 0] * q[:, 3] + q[:, 1] * q[:, 2]), 1 - 2 * (q[:, 2] ** 2 + q[:, 3] ** 2))
    c, s = np.cos(yaw), np.sin(yaw)
    return np.stack([c * v[:, 0] - s * v[:, 1], s * v[:, 0] + c * v[:, 1], v[:, 2]], -1)


def test_heading_rotation_against_float64():
    """Bound: cs and sn are each a few products and sums of quaternion components of magnitude <= 1 (4 roundings), the normalisation adds a
    square root and a division (3 more), the rotation two products and a sum per component (3): below 16 roundings of 2^-24 relative to the
    vector's length, whatever the order."""
    from kbot_joystick_amd.host.push import heading_rotate
    rng = np.random.default_rng(3)
    q = rng.normal(size=(256, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[0], q[1], q[2] = (1, 0, 0, 0), (math.cos(0.25 * math.pi), 0, 0, math.sin(0.25 * math.pi)), (0, 0, 0, 1)      # yaw 0, 90, 180 degrees
    q = q.astype(np.float32)
    v = rng.uniform(-200, 200, (256, 3)).astype(np.float32)
    v[:3] = (100, 0, 5)
    got = heading_rotate(torch.from_numpy(q), torch.from_numpy(v)).numpy().astype(np.float64)
    want = _yaw_rotate64(q, v)
    bound = 16 * 2.0 ** -24 * np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    assert (np.abs(got - want) <= bound).all(), np.abs(got - want).max()
    assert np.allclose(got[0], (100, 0, 5), atol=1e-4) and np.allclose(got[1], (0, 100, 5), atol=1e-4) and np.allclose(got[2], (-100, 0, 5), atol=1e-4)   # 0 degrees pushes forward
    up = heading_rotate(torch.tensor([[math.sqrt(0.5), 0.0, math.sqrt(0.5), 0.0]]), torch.tensor([[1.0, 2.0, 3.0]]))   # pitched 90 degrees: cs = sn = 0 up to rounding
    assert torch.isfinite(up).all()


class _Recorder:
    """Stands in for a Context: keeps what apply_events sends to kbj_env_set_push."""
    def __init__(self):
        self.calls = []

    def env_set_push(self, mask, wrench, steps, next=None):
        self.calls.append(tuple(None if t is None else t.clone() for t in (mask, wrench, steps, next)))


class _Rows:
    def __init__(self, T, N):
        self.actor_obs, self.critic_obs, self.aux = torch.zeros(T + 1, N, L.LD_ACTOR), torch.zeros(T + 1, N, L.LD_CRITIC), torch.zeros(T + 1, N, X["SIZE"])


def test_scripted_push_schedule():
    """Rows 0 .. 5 of four envs, the push on row 3 for 4 steps; env 2's episode ends in step 1 (it is fresh on row 2), env 0's in step 2 (fresh on
    the push row itself). Expected calls: row 0 - every env, zero wrench, next = NEVER; row 1 - nobody; row 2 - env 2 alone; row 3 - every
    env, its wrench turned by its own yaw; rows 4, 5 - nobody."""
    from kbot_joystick_amd.host.push import ScriptedPush
    from kbot_joystick_amd.host.user_terms import Step, UserTerms
    T, N = 5, 4
    tr, ctx = _Rows(T, N), _Recorder()
    tr.aux[:, :, X["BQUAT"]] = 1.0                                             # heading along x ...
    half = math.sqrt(0.5)
    tr.aux[2, 1, X["BQUAT"]], tr.aux[2, 1, X["BQUAT"] + 3] = half, half        # ... but env 1 faces +y when the push comes (row 3 reads the record of step 2)
    tr.aux[1, 2, X["DONE"]], tr.aux[2, 0, X["DONE"]] = -1.0, 1.0
    local = torch.zeros(N, 6); local[:, 0] = torch.tensor([50.0, 100.0, 150.0, 0.0]); local[:, 5] = 2.0
    term = ScriptedPush(local, torch.full((N,), 4.0), push_row=3)
    terms = UserTerms(events={"push": term})
    assert terms and not UserTerms()
    terms.bind(5, 0, torch.device("cpu"), compiler.load_model("kbot-headless"), L.NOBS_ACTOR, L.NOBS_CRITIC)
    for row in range(T + 1):
        terms.run_hooks(ctx, tr, row, 100 + row, [terms.apply_events])
    assert len(ctx.calls) == T + 1
    never = [L.PUSH_NEVER] * N
    masks = [c[0].tolist() for c in ctx.calls]
    assert masks == [[1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]]
    for row, (mask, wrench, steps, nxt) in enumerate(ctx.calls):
        assert nxt[mask != 0].tolist() == never[:int(mask.sum())] and mask.dtype == wrench.dtype == steps.dtype == nxt.dtype == torch.float32
        if row != 3:
            assert not wrench.any() and not steps.any()
    _, wrench, steps, _ = ctx.calls[3]
    assert steps.tolist() == [4.0] * N
    assert torch.allclose(wrench[0], torch.tensor([50.0, 0, 0, 0, 0, 2.0])) and torch.allclose(wrench[2], torch.tensor([150.0, 0, 0, 0, 0, 2.0]))
    assert torch.allclose(wrench[1], torch.tensor([0.0, 100.0, 0, 0, 0, 2.0]), atol=1e-4)           # forward for env 1 is +y
    assert not wrench[3, :3].any()                                                                   # the zero-force control case is still "pushed"


def test_later_event_terms_win_and_none_sends_nothing():
    from kbot_joystick_amd.host.traj_view import PushRequest
    from kbot_joystick_amd.host.user_terms import UserTerms
    N = 4

    def first(state, st, level, rng):
        return PushRequest(torch.tensor([True, True, False, False]), torch.full((N, 6), 1.0), torch.full((N,), 3.0), torch.full((N,), 9.0)), (0 if st is None else st) + 1

    def second(state, st, level, rng):
        return PushRequest(torch.tensor([False, True, True, False]), torch.full((N, 6), 2.0), torch.full((N,), 5.0)), st

    quiet = lambda state, st, level, rng: (None, st)
    tr = _Rows(1, N)
    model = compiler.load_model("kbot-headless")
    ctx, terms = _Recorder(), UserTerms(events={"quiet": quiet})
    terms.bind(5, 0, torch.device("cpu"), model, L.NOBS_ACTOR, L.NOBS_CRITIC)
    terms.run_hooks(ctx, tr, 0, 0, [terms.apply_events])
    assert ctx.calls == []
    ctx, terms = _Recorder(), UserTerms(events={"a": first, "quiet": quiet, "b": second})
    terms.bind(5, 0, torch.device("cpu"), model, L.NOBS_ACTOR, L.NOBS_CRITIC)
    terms.run_hooks(ctx, tr, 0, 0, [terms.apply_events])
    terms.run_hooks(ctx, tr, 1, 1, [terms.apply_events])
    assert terms.event_state_of(ctx)["a"] == 2 and terms.event_state_of(ctx)["b"] is None          # a term without initial_event_state carries what it returns
    (m0, w0, s0, n0), (m1, w1, s1, n1) = ctx.calls[:2]                             # envs without a `next` first, then those with one
    assert len(ctx.calls) == 4 and n0 is None and m0.tolist() == [0, 1, 1, 0] and m1.tolist() == [1, 0, 0, 0]
    assert w0[:, 0].tolist() == [1, 2, 2, 0] and s0.tolist() == [3, 5, 5, 0] and n1.tolist()[0] == 9


def test_table_and_case_summary():
    from kbot_joystick_amd.host.push import DEFAULT_TOLERANCES, case_summary, format_push_table
    vec = np.zeros(S["SIZE"])
    vec[S["COUNT"] + O["VOID"]], vec[S["COUNT"] + O["FELL"]], vec[S["COUNT"] + O["RECOVERED"]], vec[S["COUNT"] + O["CENSORED"]] = 1, 1, 2, 1
    vec[S["REC_SUM"]], vec[S["REC_SUMSQ"]], vec[S["REC_MAX"]] = 30, 500, 20
    vec[S["PEAK_SUM"] + 2], vec[S["PEAK_MAX"] + 2], vec[S["PEAK_SUM"]], vec[S["PEAK_MAX"]] = 0.8, 0.4, 2.0, 1.0
    x = case_summary(vec, 0.02)
    assert (x["valid"], x["void"], x["fell_frac"], x["recovered_frac"], x["unrecovered_frac"], x["censored_frac"]) == (4, 1, 0.25, 0.5, 0.0, 0.25)
    assert x["recovery_s_mean"] == pytest.approx(0.3) and x["recovery_s_max"] == pytest.approx(0.4)
    assert (x["peak_tilt_mean"], x["peak_tilt_max"], x["peak_lin_vel_err_mean"], x["peak_lin_vel_err_max"]) == (0.2, 0.4, 0.5, 1.0)
    empty = case_summary(np.zeros(S["SIZE"]), 0.02)
    assert empty["valid"] == 0 and all(math.isnan(empty[k]) for k in empty if k not in ("valid", "void"))
    assert set(DEFAULT_TOLERANCES) == set(constants.TRACKING_ERROR_NAMES)
    settings = dict(duration=0.2, push_at=2.0, window=3.0, hold=0.5, command=(0.0,) * 16, torque=(0.0,) * 3, tolerances=dict(DEFAULT_TOLERANCES), repeats=5)
    text = format_push_table([dict(force=150.0, direction_deg=90.0, **settings, **x), dict(force=0.0, direction_deg=0.0, **settings, **empty)])
    lines = text.splitlines()
    assert len(lines) == 4 and "settings, not measured thresholds" in lines[0] and "tilt_err<=0.03" in lines[0] and "arm_sq_err<=inf" in lines[0]
    assert lines[2].split()[:5] == ["150.0", "90.0", "4", "1", "0.250"] and "nan" in lines[3]
    assert format_push_table([]).count("\n") == 0
