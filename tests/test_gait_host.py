"""Gait statistics, the parts that need no GPU: the layout mirrors, the table of rules that the synthetic problems of
tests/test_gpu_gait_stats.py fire (asserted on the reference alone, so that no GPU case can pass by leaving a branch out), the scan pinned on
hand-computed cases and on a closed-form periodic gait, two calls against one, combining vectors, the scalars, the pooled sweep entry and the
table, the config field and the checkpoint members."""
import dataclasses
import math
import os

import numpy as np
import pytest

from kbot_joystick_amd.spec import constants, layout as L
from tests import gait_ref as GR

G, F, A, E, X, M = L.GAIT, L.GFOOT, L.GACC, L.GENV, L.AUX, L.CMODE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.02


def test_layout_mirrors_the_header():
    # (values against the header: tests/test_abi_mirror.py)
    assert M["COUNT"] * G["MODE_STRIDE"] == G["EPISODES"] < G["SIZE"] == 256 and G["FOOT"] + 2 * G["FOOT_STRIDE"] == G["MODE_STRIDE"] == 40
    assert F["SIZE"] == G["FOOT_STRIDE"] and sorted(v for k, v in F.items() if k != "SIZE") == list(range(16))
    assert A["SIZE"] == 16 and A["PEAK"] < A["FOOT_STRIDE"] and 2 * A["FOOT_STRIDE"] == A["RUNNING"] and A["LAST_TD"] == 13
    assert E["SIZE"] == 24 and E["FOOT"] + 2 * E["FOOT_STRIDE"] == E["SIZE"]
    assert L.gait_slot(2, "TORQUE_MAX") == 86 and L.gait_slot(1, "FORCE_MAX", 1) == 40 + 8 + 16 + 14
    kbj = open(os.path.join(ROOT, "include", "kbj.h")).read()
    assert "int kbj_gait_stats(kbj_ctx* ctx, const kbj_traj* traj, float* acc_d, double* stats_d, float* env_d);" in kbj
    from kbot_joystick_amd.host import binding as B
    assert "kbj_gait_stats" in B.SIGNATURES and len(B.SIGNATURES["kbj_gait_stats"][1]) == 5


# which rules a shape can fire at all: one env and two rows (1, 1) hold neither a phase that ends nor a planted env
FIRED = {shape: set(GR.RULES) for shape in GR.SHAPES if shape != (1, 1)}


def test_every_rule_fires_in_every_shape_the_gpu_test_uses():
    """The fired table, from the reference alone. Every shape but (1, 1) fires every rule of the scan over its two calls; (1, 1) is a launch
    with one live lane and one row, where the reference's own two rows say what happens."""
    assert len(GR.RULES) == 15
    for T, N in GR.SHAPES:
        ref = GR.reference(T, N)
        fired = ref[0][5] | ref[1][5]
        print(f"T={T} N={N}: fired {sorted(fired)}")
        if (T, N) == (1, 1):
            assert ref[0][2][G["EPISODES"]] == 1 and sum(ref[0][2][m * G["MODE_STRIDE"] + G["ROWS"]] for m in range(M["COUNT"])) == 1
            continue
        assert fired == FIRED[(T, N)], (T, N, FIRED[(T, N)] - fired)
        assert "call_starts_an_episode_from_the_carry" in ref[1][5] and "counted_phase_spans_the_call_boundary" in ref[1][5] and "run_capped" in ref[0][5]
        rows = sum(ref[0][2][m * G["MODE_STRIDE"] + G["ROWS"]] for m in range(M["COUNT"]))
        assert rows == T * N and all(ref[0][2][m * G["MODE_STRIDE"] + G["ROWS"]] + ref[1][2][m * G["MODE_STRIDE"] + G["ROWS"]] > 0 for m in range(M["COUNT"]))     # all six modes
        assert ref[0][2][L.gait_slot(M["OMNI"], "STANCE_MAX", 0)] == 2.0 ** 24 and ref[0][2][L.gait_slot(M["OMNI"], "STANCE_SUMSQ", 0)] >= 2.0 ** 48     # env 1's capped stance


def _rows(T, contact, z=None, done=None, cmd=None, force=50.0, ctrl=None):
    """aux [T, 1, 72] of one env from per-row contact pairs, heights, DONE, commands and a constant torque vector."""
    aux = np.zeros((T, 1, X["SIZE"]), np.float32)
    aux[:, 0, X["TOUCH"]:X["TOUCH"] + 2] = np.where(np.array(contact, bool), force, 0.0)
    aux[:, 0, X["LFZ"]], aux[:, 0, X["RFZ"]] = (0.04, 0.04) if z is None else np.array(z, np.float32).T
    if done is not None:
        aux[:, 0, X["DONE"]] = done
    aux[:, 0, X["CMD"]] = 0.5
    if cmd is not None:
        aux[:, 0, X["CMD"]:X["CMD"] + L.NCMD] = cmd
    if ctrl is not None:
        aux[:, 0, X["CTRL"]:X["CTRL"] + L.NU] = ctrl
    return aux


FWD = M["FORWARD"]
S = lambda name, foot=None, mode=FWD: L.gait_slot(mode, name, foot)


def test_hand_computed_supports_forces_and_torques():
    """T = 6, forward: rows (1,1) (1,0) (0,0) (0,1) (1,1) (1,1), torques of 3 on every joint, forces 50 N: 3 double, 2 single, 1 flight; left
    foot 4 contact rows, right 4; torque_sq = 6 * 20 * 9; nothing counted as a swing (every ended phase began on row 0 or was the first)..."""
    aux = _rows(6, [(1, 1), (1, 0), (0, 0), (0, 1), (1, 1), (1, 1)], ctrl=3.0)
    aux[3, 0, X["TOUCH"] + 1] = 80.0
    acc = np.zeros((1, A["SIZE"]), np.float32)
    st, mags, env, _ = GR.gait_ref(acc, aux, 6)
    assert [st[S(k)] for k in ("ROWS", "DOUBLE", "SINGLE", "FLIGHT", "REPEATS", "TORQUE_SQ", "TORQUE_MAX")] == [6, 3, 2, 1, 0, 1080.0, 3.0]
    assert (st[S("CONTACT_ROWS", 0)], st[S("CONTACT_ROWS", 1)], st[S("FORCE_SUM", 0)], st[S("FORCE_SUM", 1)], st[S("FORCE_MAX", 1)]) == (4, 4, 200.0, 230.0, 80.0)
    # right: lift-off on row 1 (first phase: no duration), touchdown on row 3 (a counted swing of 2 rows); left: lift-off on row 2 (first phase), touchdown on row 4 (2 rows)
    assert [st[S(k, 1)] for k in ("TOUCHDOWNS", "LIFTOFFS", "SWING_N", "SWING_SUM", "SWING_SUMSQ", "SWING_MAX", "STANCE_N")] == [1, 1, 1, 2, 4, 2, 0]
    assert [st[S(k, 0)] for k in ("TOUCHDOWNS", "LIFTOFFS", "SWING_N", "SWING_SUM", "SWING_MAX", "STANCE_N")] == [1, 1, 1, 2, 2, 0]
    assert st[G["EPISODES"]] == 1 and st[S("REPEATS")] == 0
    assert env[0, :8].tolist() == [6, 3, 2, 1, 0, 1080.0, 3.0, 0] and env[0, 8:16].tolist() == [1, 1, 2, 0, 0, 0, 0, 50.0] and env[0, 16:].tolist() == [1, 1, 2, 0, 0, 0, 0, 80.0]
    assert acc[0].tolist() == [1, 2, 1, np.float32(0.04), 0, 0, 1, 3, 1, np.float32(0.04), 0, 0, 1, 0, 0, 0]      # left: stance of 2 rows since row 4; right: 3 since row 3; last touchdown left


def test_hand_computed_clearance_hops_and_episode_ends():
    """T = 6, the left foot hopping with the right in the air: down, up (z 0.10, 0.12 over a stance height of 0.04), up, down, up, down. The first
    swing is counted (it began after the first phase): 2 rows, clearance 0.12 - 0.04; the second, 1 row, ends in a repeat. Then DONE cuts."""
    z = [(0.04, 0.3), (0.10, 0.3), (0.12, 0.3), (0.05, 0.3), (0.02, 0.3), (0.05, 0.3)]
    aux = _rows(6, [(1, 0), (0, 0), (0, 0), (1, 0), (0, 0), (1, 0)], z=z)
    acc = np.zeros((1, A["SIZE"]), np.float32)
    st, mags, env, _ = GR.gait_ref(acc, aux, 6)
    rise = float(np.float32(0.12) - np.float32(0.04))
    assert [st[S(k, 0)] for k in ("TOUCHDOWNS", "LIFTOFFS", "SWING_N", "SWING_SUM", "SWING_SUMSQ", "SWING_MAX", "STANCE_N", "STANCE_SUM", "STANCE_MAX")] == [2, 2, 2, 3, 5, 2, 1, 1, 1]
    assert st[S("CLEAR_MAX", 0)] == rise and abs(st[S("CLEAR_SUM", 0)] - rise) < 1e-15 and st[S("REPEATS")] == 1       # the second swing stays below 0.05: clearance 0
    assert st[S("FLIGHT")] == 3 and st[S("SINGLE")] == 3 and st[S("TOUCHDOWNS", 1)] == 0 and st[S("CONTACT_ROWS", 1)] == 0
    assert acc[0, A["LAST_TD"]] == 0 and acc[0, A["FOOT_STRIDE"] + A["PEAK"]] == np.float32(np.float32(0.3) - np.float32(0.3))
    # the right foot has been in the air since the episode began: its phase is not valid, its peak is over the height of the first row
    assert (acc[0, A["FOOT_STRIDE"] + A["VALID"]], acc[0, A["FOOT_STRIDE"] + A["RUN"]]) == (0, 6)
    # an episode end drops the phase in progress, and the next row starts afresh: no event although the contact changes
    aux = _rows(4, [(1, 1), (0, 1), (0, 1), (1, 1)], done=[0, 0, -1, 0])
    acc = np.zeros((1, A["SIZE"]), np.float32)
    st = GR.gait_ref(acc, aux, 4)[0]
    assert (st[S("LIFTOFFS", 0)], st[S("TOUCHDOWNS", 0)], st[S("SWING_N", 0)], st[G["EPISODES"]]) == (1, 0, 0, 2)
    # a NaN force and a force of exactly 0.1f are no contact; the next float is
    aux = _rows(3, [(1, 1)] * 3)
    aux[:, 0, X["TOUCH"]] = (np.nan, 0.1, np.nextafter(np.float32(0.1), np.float32(1)))
    st = GR.gait_ref(np.zeros((1, A["SIZE"]), np.float32), aux, 3)[0]
    assert (st[S("SINGLE")], st[S("DOUBLE")], st[S("CONTACT_ROWS", 0)], st[S("TOUCHDOWNS", 0)]) == (2, 1, 1, 1)
    # the event lands in the mode of the row that ends the phase
    cmd = np.zeros((5, L.NCMD), np.float32)
    cmd[:3, 0], cmd[3:, 1] = 0.5, 0.25
    st = GR.gait_ref(np.zeros((1, A["SIZE"]), np.float32), _rows(5, [(1, 1), (0, 1), (1, 1), (0, 1), (1, 1)], cmd=cmd), 5)[0]
    assert st[S("TOUCHDOWNS", 0)] == 1 and st[S("TOUCHDOWNS", 0, M["SIDEWAYS"])] == 1 and st[S("STANCE_N", 0, M["SIDEWAYS"])] == 1 and st[S("SWING_N", 0, M["SIDEWAYS"])] == 1
    # the cap: a stance that has lasted 2^24 - 1 rows, three more, a lift-off
    acc = np.zeros((1, A["SIZE"]), np.float32)
    acc[0, [A["CON"], A["RUN"], A["VALID"], A["RUNNING"]]] = (1, 2.0 ** 24 - 1, 1, 1)
    st = GR.gait_ref(acc, _rows(4, [(1, 0), (1, 0), (1, 0), (0, 0)]), 4)[0]
    assert (st[S("STANCE_SUM", 0)], st[S("STANCE_SUMSQ", 0)], st[S("STANCE_MAX", 0)]) == (2.0 ** 24, 2.0 ** 48, 2.0 ** 24)


@pytest.mark.parametrize("swing,stance", [(3, 5), (4, 4), (2, 7)])
def test_closed_form_periodic_gait(swing, stance):
    """Both feet with period p + s, the right half a period late (rounded down), over 12 periods: once the first phases are out, every swing
    lasts s rows and every stance p rows, so duty = p / (p + s) exactly, and the step rate tends to 2 / ((p + s) dt)."""
    from kbot_joystick_amd.host.gait import gait_scalars
    period, T = swing + stance, 12 * (swing + stance)
    contact = [((t % period) < stance, ((t + period // 2) % period) < stance) for t in range(T)]
    z = [(0.04 if c[0] else 0.09, 0.04 if c[1] else 0.11) for c in contact]
    st = GR.gait_ref(np.zeros((1, A["SIZE"]), np.float32), _rows(T, contact, z=z, ctrl=2.0), T)[0]
    for f in range(2):
        assert st[S("SWING_SUM", f)] == swing * st[S("SWING_N", f)] and st[S("STANCE_SUM", f)] == stance * st[S("STANCE_N", f)]
        assert st[S("SWING_MAX", f)] == swing and st[S("STANCE_MAX", f)] == stance and st[S("SWING_N", f)] >= 10 and st[S("STANCE_N", f)] >= 10
    sc = gait_scalars(st, DT)
    for side, rise in (("left", np.float32(0.09) - np.float32(0.04)), ("right", np.float32(0.11) - np.float32(0.04))):
        assert abs(sc[f"gait/forward/{side}_swing_s_mean"] - swing * DT) < 1e-12 and sc[f"gait/forward/{side}_swing_s_std"] < 1e-7 and sc[f"gait/forward/{side}_stance_s_max"] == stance * DT
        assert abs(sc[f"gait/forward/{side}_clearance_m_mean"] - float(rise)) < 1e-12 and sc[f"gait/forward/{side}_clearance_m_max"] == float(rise)
        # the counted phases alone: whole periods but for one phase at either end
        n_sw, n_st = st[S("SWING_N", 0 if side == "left" else 1)], st[S("STANCE_N", 0 if side == "left" else 1)]
        assert abs(n_sw - n_st) <= 1 and sc[f"gait/forward/{side}_duty"] == stance * n_st / (stance * n_st + swing * n_sw)
        if n_sw == n_st:
            assert sc[f"gait/forward/{side}_duty"] == stance / period
        assert sc[f"gait/forward/{side}_force_n_mean"] == 50.0 == sc[f"gait/forward/{side}_force_n_max"]
    touchdowns = st[S("TOUCHDOWNS", 0)] + st[S("TOUCHDOWNS", 1)]
    assert 2 * 12 - 2 <= touchdowns <= 2 * 12 and sc["gait/forward/step_rate_hz"] == touchdowns / (T * DT)
    assert abs(sc["gait/forward/step_rate_hz"] - 2 / (period * DT)) <= 2 / (T * DT)                  # two touchdowns short at the most
    assert sc["gait/forward/swing_asymmetry"] == 0.0 and sc["gait/forward/repeat_frac"] == 0.0 and sc["gait/forward/torque_rms"] == 2.0 and sc["gait/forward/torque_max"] == 2.0
    assert abs(sc["gait/forward/double_support_frac"] + sc["gait/forward/single_support_frac"] + sc["gait/forward/flight_frac"] - 1) < 1e-15


@pytest.mark.parametrize("T,N", GR.SHAPES[1:4])
def test_two_calls_equal_one_call_of_twice_the_rows(T, N):
    from kbot_joystick_amd.host import dist as D
    P, ref = GR.problems(T, N), GR.reference(T, N)
    both = np.concatenate([P.calls[0][:T], P.calls[1][:T]])
    acc = P.acc0.copy()
    st, mags, env, _ = GR.gait_ref(acc, both, 2 * T)
    assert acc.tobytes() == ref[1][1].tobytes()                                          # the carry
    joined = D.combine_gait_stats([ref[0][2], ref[1][2]])
    ex = GR.exact_slots()
    assert np.array_equal(joined[ex], st[ex])                                            # counts, duration sums and squares, maxima
    assert (np.abs(joined[~ex] - st[~ex]) <= 1e-12 * mags[~ex]).all()                    # float64 sums: associative to a rounding
    whole = [k for k in range(E["SIZE"]) if k not in (G["TORQUE_SQ"], 8 + E["CLEAR_SUM"], 16 + E["CLEAR_SUM"])]
    e2 = ref[0][4].astype(np.float64) + ref[1][4]
    for k in (G["TORQUE_MAX"], 8 + E["CLEAR_MAX"], 8 + E["FORCE_MAX"], 16 + E["CLEAR_MAX"], 16 + E["FORCE_MAX"]):
        e2[:, k] = np.maximum(ref[0][4][:, k], ref[1][4][:, k])
    assert np.array_equal(e2[:, whole], env[:, whole].astype(np.float64))


def test_combine_of_rank_vectors_is_the_vector_of_the_union():
    from kbot_joystick_amd.host import dist as D
    import torch
    T, N = GR.SHAPES[2]
    P = GR.problems(T, N)
    whole, mags = GR.reference(T, N)[0][2], GR.reference(T, N)[0][3]
    halves = [GR.gait_ref(P.acc0[s].copy(), P.calls[0][:, s], T)[0] for s in (slice(0, N // 2), slice(N // 2, N))]
    assert not np.array_equal(halves[0], halves[1])
    GR.assert_stats_match(D.combine_gait_stats(halves), whole, mags)
    e = D.empty_gait_stats()
    assert e.shape == (G["SIZE"],) and not e.any() and np.array_equal(D.combine_gait_stats([]), e) and np.array_equal(D.combine_gait_stats([whole, e]), whole)
    hi = np.zeros(G["SIZE"], bool)
    hi[D.GAIT_STATS.hi] = True
    assert hi.sum() == M["COUNT"] * 9 and np.array_equal(D.combine_gait_stats(halves)[hi], np.maximum(*halves)[hi]) and (whole[hi] > 0).any()
    assert np.array_equal(D.reduce_gait_stats(torch.from_numpy(whole), 1).numpy(), whole)       # one rank: no collective


def test_scalars_omit_what_has_no_denominator():
    from kbot_joystick_amd.host import dist as D
    from kbot_joystick_amd.host.gait import gait_scalars
    assert gait_scalars(D.empty_gait_stats(), DT) == {}
    v = D.empty_gait_stats()
    side = M["SIDEWAYS"]
    v[S("ROWS", mode=side)], v[S("DOUBLE", mode=side)], v[S("SINGLE", mode=side)], v[S("TORQUE_SQ", mode=side)], v[S("TORQUE_MAX", mode=side)] = 10, 4, 6, 10 * 20 * 4.0, 9.0
    v[S("CONTACT_ROWS", 0, side)], v[S("FORCE_SUM", 0, side)], v[S("FORCE_MAX", 0, side)] = 8, 800.0, 250.0
    s = gait_scalars(v, DT, "x/")
    assert s == {"x/sideways/double_support_frac": 0.4, "x/sideways/single_support_frac": 0.6, "x/sideways/flight_frac": 0.0, "x/sideways/step_rate_hz": 0.0,
                 "x/sideways/torque_rms": 2.0, "x/sideways/torque_max": 9.0, "x/sideways/left_force_n_mean": 100.0, "x/sideways/left_force_n_max": 250.0}
    v[S("TOUCHDOWNS", 0, side)], v[S("TOUCHDOWNS", 1, side)], v[S("REPEATS", mode=side)] = 3, 1, 1
    v[S("SWING_N", 0, side)], v[S("SWING_SUM", 0, side)], v[S("SWING_SUMSQ", 0, side)], v[S("SWING_MAX", 0, side)], v[S("CLEAR_SUM", 0, side)], v[S("CLEAR_MAX", 0, side)] = 2, 10, 52, 6, 0.1, 0.07
    v[S("SWING_N", 1, side)], v[S("SWING_SUM", 1, side)], v[S("SWING_SUMSQ", 1, side)], v[S("SWING_MAX", 1, side)] = 1, 15, 225, 15
    v[S("STANCE_N", 0, side)], v[S("STANCE_SUM", 0, side)], v[S("STANCE_SUMSQ", 0, side)], v[S("STANCE_MAX", 0, side)] = 1, 30, 900, 30
    s = gait_scalars(v, DT, "x/")
    want = {"x/sideways/step_rate_hz": 4 / (10 * DT), "x/sideways/repeat_frac": 0.25, "x/sideways/left_swing_s_mean": 5 * DT, "x/sideways/left_swing_s_std": 1 * DT,
            "x/sideways/left_swing_s_max": 6 * DT, "x/sideways/left_clearance_m_mean": 0.05, "x/sideways/left_clearance_m_max": 0.07, "x/sideways/left_duty": 0.75,
            "x/sideways/left_stance_s_mean": 30 * DT, "x/sideways/left_stance_s_std": 0.0, "x/sideways/right_swing_s_mean": 15 * DT, "x/sideways/right_duty": 0.0,
            "x/sideways/swing_asymmetry": (5 - 15) / (5 + 15)}
    for k, x in want.items():
        assert abs(s[k] - x) < 1e-12, (k, s[k], x)
    assert "x/sideways/right_stance_s_mean" not in s and "x/sideways/right_force_n_mean" not in s and not any("forward" in k for k in s)


def test_pooled_entry_and_table():
    from kbot_joystick_amd.host.gait import GAIT_TABLE_COLUMNS, format_gait_table, pool_gait_rows
    rows = np.zeros((2, E["SIZE"]), np.float32)
    rows[:, G["ROWS"]], rows[:, G["DOUBLE"]], rows[:, G["SINGLE"]], rows[:, G["TORQUE_SQ"]] = 50, (10, 20), (40, 30), 50 * 20 * 9.0
    rows[0, 8:16] = (4, 3, 30, 3, 60, 0.15, 0.08, 300.0)
    rows[1, 8:16] = (2, 1, 10, 2, 40, 0.05, 0.09, 200.0)
    x = pool_gait_rows(rows, DT)
    assert x["left_swing_s"] == 10 * DT and x["left_stance_s"] == 20 * DT and abs(x["left_clearance_m_mean"] - 0.05) < 1e-8 and x["left_clearance_m_max"] == float(np.float32(0.09))
    assert x["left_force_n_max"] == 300.0 and x["step_rate_hz"] == 6 / (100 * DT) and (x["double_support_frac"], x["single_support_frac"], x["flight_frac"]) == (0.3, 0.7, 0.0)
    assert x["torque_rms"] == 3.0 and x["repeat_frac"] == 0.0 and math.isnan(x["right_swing_s"]) and math.isnan(x["right_clearance_m_mean"]) and x["right_force_n_max"] == 0.0
    entries = [dict(command=(0.5,) + (0.0,) * 15, mode="forward", failures_per_s=0.25, **x), dict(command=(0.0,) * 16, mode="stand", failures_per_s=0.0, **pool_gait_rows(rows[:0], DT))]
    text = format_gait_table(entries).splitlines()
    assert len(text) == 3 and all(title in text[0] for title, _ in GAIT_TABLE_COLUMNS)
    assert text[1].startswith("xvel=+0.50") and "forward" in text[1] and "0.200" in text[1] and "300.000" in text[1] and " - " in text[1] + " "
    assert text[2].startswith("(zero)") and "stand" in text[2]


def test_config_field_and_checkpoint_members(tmp_path, monkeypatch):
    from kbot_joystick_amd.host import ckpt, dist as D
    from kbot_joystick_amd.host.task import HumanoidWalkingTaskConfig, launch_config
    monkeypatch.delenv("KBJ_GAIT_STATS", raising=False)
    assert HumanoidWalkingTaskConfig().gait_stats is False and launch_config().gait_stats is False
    monkeypatch.setenv("KBJ_GAIT_STATS", "1")
    assert HumanoidWalkingTaskConfig().gait_stats is True and HumanoidWalkingTaskConfig(gait_stats=False).gait_stats is False
    monkeypatch.setenv("KBJ_GAIT_STATS", "0")
    assert HumanoidWalkingTaskConfig().gait_stats is False
    cfg = launch_config(gait_stats=True, hidden_size=16, depth=1)
    d = dataclasses.asdict(cfg)
    d["action_latency_range"] = tuple(d["action_latency_range"])
    assert d["gait_stats"] is True and HumanoidWalkingTaskConfig(**d) == cfg
    old = {k: v for k, v in d.items() if k != "gait_stats"}                            # a config member written before the field existed
    assert HumanoidWalkingTaskConfig(**old).gait_stats is False
    P = sum(L.param_count(16, 1))
    p = np.arange(P, dtype=np.float32)
    d["action_latency_range"] = list(d["action_latency_range"])
    acc = np.random.default_rng(0).uniform(0, 9, (4, A["SIZE"])).astype(np.float32)
    total = D.empty_gait_stats()
    total[G["ROWS"]], total[G["TORQUE_SQ"]] = 7, 0.1 + 0.2
    path = str(tmp_path / "new.bin")
    ckpt.save_ckpt(path, p, p, p, 1, 16, 1, dict(num_steps=1), d, dict(es=np.zeros((4, L.ES["SIZE"]), np.float32), gait_acc=acc, gait_total=total))
    z = ckpt.load_ckpt(path, "all")
    assert z["config"]["gait_stats"] is True
    assert z["extras"]["gait_acc"].dtype == np.float32 and np.array_equal(z["extras"]["gait_acc"], acc)
    assert z["extras"]["gait_total"].dtype == np.float64 and np.array_equal(z["extras"]["gait_total"], total)
