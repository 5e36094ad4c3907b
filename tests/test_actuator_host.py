"""Actuator statistics without a GPU: the layout mirrors, the numpy restatement (tests/actuator_ref.py) against answers computed by hand, the
synthetic problems' coverage, the levels of the committed robot, the scalars and tables on a hand-made vector, the record_state guard, the
slot rule and its reduction over two gloo ranks, and the checkpoint round trip of the carrier's state."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from kbot_joystick_amd.spec import constants, layout as L
from tests import actuator_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, J, A, E, X, Q, M = L.ACT, L.AJNT, L.AACC, L.AENV, L.AUX, L.QSTATE, L.CMODE
NU = L.NU


def test_layout_mirrors_the_header():
    # (values against the header: tests/test_abi_mirror.py)
    assert M["COUNT"] * V["MODE_STRIDE"] == V["EPISODES"] < V["SIZE"] == 1792 and V["SIZE"] % 256 == 0 and V["JOINT"] + NU * J["SIZE"] <= V["MODE_STRIDE"] == 256
    assert J["SIZE"] == 12 and sorted(v for k, v in J.items() if k != "SIZE") == list(range(12)) and A == dict(PREV=0, RUNNING=20, SIZE=24) and E["SIZE"] == 12
    assert L.act_slot(2, "ANY_STOP_ROWS") == 516 and L.act_slot(1, "POW_MAX", 19) == 256 + 8 + 12 * 19 + 8
    kbj = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kbj.h")).read(), flags=re.S)
    assert re.search(r"int kbj_actuator_stats\(kbj_ctx\* ctx, const kbj_traj\* traj, const kbj_actuator_levels\* levels,\s*float\* acc_d\s*, double\* stats_d\s*, float\* env_d\s*\);", kbj)
    from kbot_joystick_amd.host import binding as B
    import ctypes
    assert "kbj_actuator_stats" in B.SIGNATURES and len(B.SIGNATURES["kbj_actuator_stats"][1]) == 6 and ctypes.sizeof(B.ActuatorLevels) == 4 * NU * 4
    src = open(os.path.join(ROOT, "kbot-joystick_amd", "csrc", "kbj_actuator_stats.h")).read()
    assert f"ACT_ENVS = {AR.ENVS};" in src and f"ACT_TC = {AR.CHUNK};" in src            # the shapes straddle the kernel's workgroup and chunk


def _hand_problem():
    """3 rows x 2 envs; only joints 0 and 1 move. Levels: torque 10 everywhere, speed 2 on joint 0 and none elsewhere, stops at -1 / +1."""
    lv = dict(tau_level=np.full(NU, 10, np.float32), vel_level=np.array([2.0] + [np.inf] * (NU - 1), np.float32), pos_lo=np.full(NU, -1, np.float32), pos_hi=np.full(NU, 1, np.float32))
    aux, qs, act = np.zeros((3, 2, X["SIZE"]), np.float32), np.zeros((3, 2, Q["SIZE"]), np.float32), np.zeros((3, 2, NU), np.float32)
    tau, om, q = aux[:, :, X["CTRL"]:X["CTRL"] + NU], qs[:, :, Q["QVEL"] + 6:Q["QVEL"] + 6 + NU], qs[:, :, Q["QPOS"] + 7:Q["QPOS"] + 7 + NU]
    # env 0 walks forward; its episode ends on row 1
    aux[:, 0, X["CMD"]], aux[:, 0, X["DONE"]] = 0.5, (0, -1, 0)
    aux[:, 0, X["QVEL"]], aux[:, 0, X["QVEL"] + 1] = (3, 0, -6), (4, 0, 8)
    tau[:, 0, 0], om[:, 0, 0], q[:, 0, 0], act[:, 0, 0] = (10, -12, 1), (2, 1.5, 1), (-1, 0.5, 0), (0.5, 0.75, 9)
    tau[:, 0, 1], om[:, 0, 1], q[:, 0, 1], act[:, 0, 1] = (-4, 2, 0), (0.5, -3, 0), (0.25, 1.5, 0), (-1, -1, 0)
    # env 1 stands, then turns on row 2, where a time-out ends its episode; the carry says its episode was running
    aux[2, 1, X["CMD"] + 2], aux[:, 1, X["DONE"]] = 0.3, (0, 0, 1)
    act[:, 1, 0], tau[2, 1, 1], om[2, 1, 1] = (1.5, 1.5, 3.5), 5, 2
    qs[:, :, :7], qs[:, :, Q["QVEL"]:Q["QVEL"] + 6], qs[:, :, Q["QPOS_KIN"]:] = 99, -99, 77     # what sits around the joints is not read
    acc = np.zeros((2, A["SIZE"]), np.float32)
    acc[1, A["RUNNING"]], acc[1, A["PREV"]], acc[:, A["RUNNING"] + 1:] = 1, 1.0, 7
    return lv, aux, qs, act, acc


def test_the_restatement_gives_the_answers_computed_by_hand():
    lv, aux, qs, act, acc = _hand_problem()
    stats, mags, env = AR.actuator_ref(acc, aux, qs, act, 3, lv)
    want = np.zeros(V["SIZE"])
    F, S, R = M["FORWARD"], M["STAND"], M["ROTATE"]
    for name, x in dict(ROWS=3, PAIRS=1, SPEED_SUM=15, ANY_TAU_ROWS=2, ANY_STOP_ROWS=2).items():
        want[L.act_slot(F, name)] = x
    j0 = dict(TAU_SQ=245, TAU_MAX=12, TAU_ROWS=2, VEL_SQ=7.25, VEL_MAX=2, VEL_ROWS=1, POW_ABS=39, POW_POS=21, POW_MAX=20, STOP_ROWS=1, DACT_SQ=0.0625, DACT_MAX=0.25)
    j1 = dict(TAU_SQ=20, TAU_MAX=4, TAU_ROWS=0, VEL_SQ=9.25, VEL_MAX=3, VEL_ROWS=0, POW_ABS=8, POW_POS=0, POW_MAX=6, STOP_ROWS=1, DACT_SQ=0, DACT_MAX=0)
    for u, block in enumerate((j0, j1)):
        for name, x in block.items():
            want[L.act_slot(F, name, u)] = x
    want[L.act_slot(S, "ROWS")], want[L.act_slot(S, "PAIRS")], want[L.act_slot(S, "DACT_SQ", 0)], want[L.act_slot(S, "DACT_MAX", 0)] = 2, 2, 0.25, 0.5
    want[L.act_slot(R, "ROWS")], want[L.act_slot(R, "PAIRS")], want[L.act_slot(R, "DACT_SQ", 0)], want[L.act_slot(R, "DACT_MAX", 0)] = 1, 1, 4, 2
    for name, x in dict(TAU_SQ=25, TAU_MAX=5, VEL_SQ=4, VEL_MAX=2, POW_ABS=10, POW_POS=10, POW_MAX=10).items():
        want[L.act_slot(R, name, 1)] = x
    want[V["EPISODES"]] = 2
    assert np.array_equal(stats, want), np.flatnonzero(stats != want)
    assert mags[L.act_slot(F, "POW_ABS", 0)] == 39 and mags[L.act_slot(F, "TAU_ROWS", 0)] == 0
    env_want = np.zeros((2, E["SIZE"]), np.float32)
    env_want[0, :11] = (3, 1, 15, 265, 47, 21, 0.0625, 2, 2, np.float32(12) / np.float32(10), 0)
    env_want[1, :11] = (3, 3, 0, 25, 10, 10, 4.25, 0, 0, 0.5, 1)
    assert np.array_equal(env, env_want), (env, env_want)
    carry = np.zeros((2, A["SIZE"]), np.float32)
    carry[0, :2], carry[0, A["RUNNING"]], carry[1, 0], carry[:, A["RUNNING"] + 1:] = (9, 0), 1, 3.5, 7
    assert np.array_equal(acc, carry)


def test_the_synthetic_problems_reach_every_slot_family_and_both_sides_of_every_level():
    live, taken, not_taken = np.zeros(V["SIZE"], bool), set(), set()
    modes, cut, kept, ties = set(), 0, 0, 0
    for T, N in AR.SHAPES:
        P, ref = AR.problems(T, N), AR.reference(T, N)
        assert P.acc0[:, A["RUNNING"] + 1:].tolist() == [[7.0] * 3] * N and len(set(P.lv["tau_level"].tolist())) == NU and np.isinf(P.lv["vel_level"]).sum() == NU // 2
        for call, (before, after, stats, mags, env) in enumerate(ref):
            live |= stats != 0
            assert (after[:, A["RUNNING"] + 1:] == 7.0).all() and (stats[~AR.used_slots()] == 0).all()
            rows = sum(stats[L.act_slot(m, "ROWS")] for m in range(M["COUNT"]))
            assert rows == T * N and (env[:, E["ROWS"]] == T).all()
            modes |= {m for m in range(M["COUNT"]) if stats[L.act_slot(m, "ROWS")] > 0}
            for k in AR.COUNTS:
                n = sum(stats[L.act_slot(m, k, u)] for m in range(M["COUNT"]) for u in range(NU))
                taken |= {k} if n > 0 else set()
                not_taken |= {k} if n < rows * NU else set()
            aux, qs, act = P.calls[call]
            done = aux[:T, :, X["DONE"]]
            if call == 1:
                cut, kept = cut + int((before[:, A["RUNNING"]] == 0).sum()), kept + int((before[:, A["RUNNING"]] != 0).sum())
            if P.planted:
                assert done[0, 0] == -1 and done[0, 1] == 1 if call == 0 else done[T - 1, 3] == 1
                peaks = np.abs(aux[:T, 7, X["CTRL"]:X["CTRL"] + NU]) / P.lv["tau_level"]
                ties += int((peaks == peaks.max()).sum() == 2 and env[7, E["PEAK_JOINT"]] == 3 and env[7, E["PEAK_FRAC"]] == 2.0)
                if call == 0:
                    # env 5, row 1: every level is met exactly and counts; row 2 is one fp32 step inside and does not
                    tau, om, q = aux[1:3, 5, X["CTRL"]:X["CTRL"] + NU], qs[1:3, 5, Q["QVEL"] + 6:Q["QVEL"] + 6 + NU], qs[1:3, 5, Q["QPOS"] + 7:Q["QPOS"] + 7 + NU]
                    assert (np.abs(tau[0]) == P.lv["tau_level"]).all() and (np.abs(tau[1]) < P.lv["tau_level"]).all()
                    assert ((np.abs(om[0]) == P.lv["vel_level"]) | np.isinf(P.lv["vel_level"])).all() and (np.abs(om[1]) < P.lv["vel_level"]).all()
                    assert ((q[0] == P.lv["pos_lo"]) | (q[0] == P.lv["pos_hi"])).all() and ((q[1] > P.lv["pos_lo"]) & (q[1] < P.lv["pos_hi"])).all()
                    only = lambda rows_: AR.actuator_ref(np.zeros((1, A["SIZE"]), np.float32), aux[rows_, 5:6], qs[rows_, 5:6], act[rows_, 5:6], 1, P.lv)[0]
                    on, inside = only(slice(1, 2)), only(slice(2, 3))
                    count = lambda v, k: sum(v[L.act_slot(m, k, u)] for m in range(M["COUNT"]) for u in range(NU))
                    assert (count(on, "TAU_ROWS"), count(on, "VEL_ROWS"), count(on, "STOP_ROWS")) == (NU, NU // 2, NU)
                    assert (count(inside, "TAU_ROWS"), count(inside, "VEL_ROWS"), count(inside, "STOP_ROWS")) == (0, 0, 0)
                    assert np.signbit(aux[1, 6, X["CTRL"]]) and np.signbit(aux[1, 6, X["CMD"]]) and AR.mode_of(aux[1, 6, X["CMD"]:X["CMD"] + L.NCMD]) == M["STAND"]
                    assert (done[1, 4], done[2, 4], done[T - 1, 2], done[T - 1, 3]) == (-1, 1, -1, 0)
    assert live[AR.used_slots()].reshape(-1).sum() > 0 and modes == set(range(M["COUNT"])) and taken == not_taken == set(AR.COUNTS)
    for k in [k for k in J if k != "SIZE"]:
        assert any(live[L.act_slot(m, k, u)] for m in range(M["COUNT"]) for u in range(NU)), k
        for u in range(NU):            # every joint is reached - but for the speed count of the joints without a speed level (+inf), which stays 0
            assert any(live[L.act_slot(m, k, u)] for m in range(M["COUNT"])) == (k != "VEL_ROWS" or u % 2 == 0), (k, u)
    for k in ("ROWS", "PAIRS", "SPEED_SUM", "ANY_TAU_ROWS", "ANY_STOP_ROWS"):
        assert all(live[L.act_slot(m, k)] for m in range(M["COUNT"])), k
    assert live[V["EPISODES"]] and cut > 0 and kept > 0 and ties == 2 * sum(AR.problems(T, N).planted for T, N in AR.SHAPES)


def test_levels_of_the_committed_robot():
    from kbot_joystick_amd.host import actuator as HA
    from kbot_joystick_amd.spec import compiler
    model = compiler.load_model("kbot-headless")
    lv = HA.actuator_levels(model)
    knee = constants.JOINT_NAMES.index("dof_left_knee_04")
    assert model.tau_limit[knee] == 84.0 and lv.tau_level[knee] == np.float32(0.9 * 84.0)
    for u in range(NU):
        lo, hi = model.dof_range[6 + u]
        assert lv.tau_level[u] == np.float32(0.9 * model.tau_limit[u]) and lv.vel_level[u] == np.inf
        assert lv.pos_lo[u] == np.float32(lo + math.radians(2.0)) and lv.pos_hi[u] == np.float32(hi - math.radians(2.0)) and lv.pos_lo[u] < lv.pos_hi[u]
    lv = HA.actuator_levels(model, torque_level=0.5, speed_limit=7.5, stop_margin_deg=0.0)
    assert lv.tau_level[knee] == 42.0 and list(lv.vel_level) == [7.5] * NU and lv.pos_lo[knee] == np.float32(model.dof_range[6 + knee][0])
    assert list(HA.actuator_levels(model, speed_limit=list(range(1, NU + 1))).vel_level) == list(range(1, NU + 1))
    wide = HA.actuator_levels(model, stop_margin_deg=179.0)            # a margin wider than the range: the band collapses to its middle
    assert all(wide.pos_lo[u] == wide.pos_hi[u] for u in range(NU))
    for bad in (dict(torque_level=0.0), dict(speed_limit=-1.0), dict(speed_limit=[1.0, 2.0]), dict(stop_margin_deg=-1.0), dict(torque_level=float("nan"))):
        with pytest.raises(ValueError):
            HA.actuator_levels(model, **bad)


def _hand_vector(model, lv):
    vec = np.zeros(V["SIZE"])
    F, S = M["FORWARD"], M["STAND"]
    vec[L.act_slot(F, "ROWS")], vec[L.act_slot(F, "PAIRS")], vec[L.act_slot(F, "SPEED_SUM")] = 100, 90, 50
    vec[L.act_slot(F, "ANY_TAU_ROWS")], vec[L.act_slot(F, "ANY_STOP_ROWS")] = 30, 5
    vec[L.act_slot(F, "POW_ABS", 0)], vec[L.act_slot(F, "POW_ABS", 3)], vec[L.act_slot(F, "POW_POS", 0)] = 2000, 1000, 1500
    vec[L.act_slot(F, "POW_MAX", 3)] = 250
    vec[L.act_slot(F, "TAU_SQ", 0)], vec[L.act_slot(F, "TAU_SQ", 3)] = 6000, 2000
    vec[L.act_slot(F, "TAU_MAX", 3)], vec[L.act_slot(F, "TAU_MAX", 4)] = 0.5 * lv.tau_level[3], 0.8 * lv.tau_level[4]
    vec[L.act_slot(F, "TAU_ROWS", 3)], vec[L.act_slot(F, "STOP_ROWS", 3)], vec[L.act_slot(F, "VEL_SQ", 3)], vec[L.act_slot(F, "VEL_MAX", 3)] = 30, 5, 400, 6
    vec[L.act_slot(F, "DACT_SQ", 0)], vec[L.act_slot(F, "DACT_SQ", 3)], vec[L.act_slot(F, "DACT_MAX", 3)] = 0.9, 0.9, 0.4
    vec[L.act_slot(S, "ROWS")], vec[L.act_slot(S, "SPEED_SUM")], vec[L.act_slot(S, "POW_ABS", 2)] = 10, 1, 40
    vec[L.act_slot(S, "TAU_MAX", 3)] = 0.25 * lv.tau_level[3]
    vec[V["EPISODES"]] = 10
    return vec


def test_scalars_and_tables_of_a_vector_made_by_hand():
    from kbot_joystick_amd.host import actuator as HA
    from kbot_joystick_amd.spec import compiler
    model = compiler.load_model("kbot-headless")
    lv = HA.actuator_levels(model)
    vec, dt = _hand_vector(model, lv), 0.02
    sc = HA.actuator_scalars(vec, model, dt, "act/")
    assert {k.split("/")[1] for k in sc} == {"forward", "stand"} and len(sc) == 20 and all(k.startswith("act/") for k in sc)
    f = {k.split("/")[2]: v for k, v in sc.items() if k.startswith("act/forward/")}
    weight = float(model.total_mass) * abs(float(model.gravity[2]))
    assert f["power_abs_w"] == 30.0 and f["power_pos_w"] == 15.0 and f["torque_rms"] == 2.0 and f["at_torque_level_frac"] == 0.3 and f["at_stop_frac"] == 0.05
    assert f["cost_of_transport"] == pytest.approx(3000.0 / (weight * 50.0), rel=1e-12) and 0.1 < f["cost_of_transport"] < 0.3      # 36 kg at 0.5 m/s on 30 W
    assert f["action_rate_rms"] == pytest.approx(math.sqrt(1.8 / (90 * NU)), rel=1e-12) and f["action_rate_max"] == 0.4
    assert f["worst_joint"] == 4.0 and f["worst_joint_frac"] == pytest.approx(0.8, rel=1e-6)
    s = {k.split("/")[2]: v for k, v in sc.items() if k.startswith("act/stand/")}
    assert s["power_abs_w"] == 4.0 and s["cost_of_transport"] != s["cost_of_transport"]            # 10 rows covered 0.02 m: no cost of transport
    assert s["action_rate_rms"] != s["action_rate_rms"] and s["action_rate_max"] != s["action_rate_max"] and s["worst_joint"] == 3.0      # no pairs: no action rate
    assert HA.actuator_scalars(np.zeros(V["SIZE"]), model, dt) == {}
    half = HA.actuator_scalars(vec, model, dt, "x/", HA.actuator_levels(model, torque_level=0.45))  # the levels the vector was taken with
    assert half["x/forward/worst_joint_frac"] == pytest.approx(1.6, rel=1e-6)
    # the per-joint table, of one mode and of all rows together
    table = HA.actuator_joint_table(vec, model, dt, M["FORWARD"])
    assert [x["joint"] for x in table] == list(constants.JOINT_NAMES)
    knee = table[3]
    assert knee["torque_rms_frac"] == pytest.approx(math.sqrt(20.0) / 84.0) and knee["torque_max_frac"] == pytest.approx(0.45, rel=1e-6) and knee["torque_level_frac"] == 0.3
    assert knee["speed_rms"] == 2.0 and knee["speed_max"] == 6.0 and knee["power_abs_w"] == 10.0 and knee["power_max_w"] == 250.0 and knee["stop_frac"] == 0.05
    assert knee["action_rate_rms"] == 0.1 and knee["action_rate_rms_per_s"] == pytest.approx(5.0)
    pooled = HA.actuator_joint_table(vec, model, dt)
    assert pooled[3]["torque_max_frac"] == pytest.approx(0.45, rel=1e-6) and pooled[2]["power_abs_w"] == 40.0 / 110.0 and pooled[3]["torque_level_frac"] == 30.0 / 110.0
    empty = HA.actuator_joint_table(vec, model, dt, M["ROTATE"])
    assert all(x != x for k, x in empty[0].items() if k != "joint")
    text = HA.format_actuator_joint_table(table)
    assert len(text.splitlines()) == NU + 1 and "dof_left_knee_04" in text and "tau max/lim" in text and "     0.450" in text
    assert "         -" in HA.format_actuator_joint_table(empty)
    # the sweep's pooling and table, from per-env records made by hand
    rows = np.zeros((2, E["SIZE"]), np.float32)
    rows[0, :11] = (50, 49, 25, 4000, 1500, 800, 0.49, 10, 0, 0.7, 8)
    rows[1, :11] = (50, 49, 25, 4000, 1500, 700, 0.49, 20, 5, 0.95, 3)
    p = HA.pool_actuator_rows(rows, model, dt)
    assert p["power_abs_w"] == 30.0 and p["power_pos_w"] == 15.0 and p["torque_rms"] == 2.0 and p["at_torque_level_frac"] == 0.3 and p["at_stop_frac"] == 0.05
    assert p["cost_of_transport"] == pytest.approx(3000.0 / (weight * 50.0), rel=1e-12) and p["action_rate_rms"] == pytest.approx(math.sqrt(0.98 / (98 * NU)), rel=1e-6)
    assert p["worst_joint"] == "dof_left_knee_04" and p["worst_joint_frac"] == pytest.approx(0.95, rel=1e-6)
    nothing = HA.pool_actuator_rows(np.zeros((0, E["SIZE"])), model, dt)
    assert nothing["worst_joint"] == "-" and nothing["power_abs_w"] != nothing["power_abs_w"]
    entries = [dict(command=(0.6,) + (0.0,) * 15, mode="forward", failures_per_s=0.0, **p), dict(command=(0.0,) * 16, mode="stand", failures_per_s=float("nan"), **nothing)]
    text = HA.format_actuator_table(entries)
    assert len(text.splitlines()) == 3 and "xvel=+0.60" in text and "(zero)" in text and "dof_left_knee_04" in text and "CoT" in text
    assert "has NOT been taken on a trained policy" in " ".join(HA.actuator_sweep.__doc__.split())


def test_the_switch_needs_the_state_record():
    from kbot_joystick_amd.host.config import HumanoidWalkingTaskConfig
    from kbot_joystick_amd.host.task import launch_config
    base = dict(num_envs=64, batch_size=64, hidden_size=64, robot="kbot-headless")
    assert HumanoidWalkingTaskConfig().actuator_stats is False and HumanoidWalkingTaskConfig().actuator_torque_level == 0.9
    with pytest.raises(ValueError, match=r"record_state=True.*262 MB"):
        launch_config(actuator_stats=True, **base).to_kbj(64)
    launch_config(actuator_stats=True, record_state=True, **base).to_kbj(64)
    launch_config(**base).to_kbj(64)
    os.environ["KBJ_ACTUATOR_STATS"] = "1"
    try:
        assert HumanoidWalkingTaskConfig().actuator_stats is True
    finally:
        del os.environ["KBJ_ACTUATOR_STATS"]


def _max_mask():
    hi = np.zeros(V["SIZE"], bool)
    for m in range(M["COUNT"]):
        for u in range(NU):
            for k in ("TAU_MAX", "VEL_MAX", "POW_MAX", "DACT_MAX"):
                hi[L.act_slot(m, k, u)] = True
    return hi


def test_combine_adds_counts_and_sums_and_takes_maxima():
    from kbot_joystick_amd.host import dist as D
    hi = _max_mask()
    assert hi.sum() == 4 * NU * M["COUNT"] and D.empty_actuator_stats().tobytes() == np.zeros(V["SIZE"]).tobytes()
    vecs = [AR.reference(*AR.SHAPES[4])[call][2] for call in range(2)] + [AR.reference(*AR.SHAPES[3])[0][2]]
    want = np.zeros(V["SIZE"])
    for v in vecs:
        want = np.where(hi, np.maximum(want, v), want + v)
    assert D.combine_actuator_stats(vecs).tobytes() == want.tobytes() and D.combine_actuator_stats([]).tobytes() == np.zeros(V["SIZE"]).tobytes()
    assert (want[hi] > 0).any() and D.combine_actuator_stats(vecs[:1]).tobytes() == vecs[0].tobytes()


def _half(rank):
    """The KBJ_ACT vector of envs [16 rank, 16 rank + 16) of the synthetic problem (11, 33), first call."""
    T, N = AR.SHAPES[4]
    P = AR.problems(T, N)
    aux, qs, act = (x[:, 16 * rank:16 * rank + 16] for x in P.calls[0])
    return AR.actuator_ref(np.zeros((16, A["SIZE"]), np.float32), aux, qs, act, T, P.lv)[0]


def _reduce_worker(rank, world, port, out):
    import torch.distributed as dist
    from kbot_joystick_amd.host import dist as D
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    mine = _half(rank)
    out[rank] = dict(mine=mine, reduced=D.reduce_actuator_stats(torch.from_numpy(mine), world).numpy())
    dist.destroy_process_group()


def test_reduce_actuator_stats_two_ranks_gloo():
    from kbot_joystick_amd.host import dist as D
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_reduce_worker, args=(2, 29573, out), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    hi = _max_mask()
    assert (r0["mine"][hi] > 0).any() and (r1["mine"][hi] > 0).any() and not np.array_equal(r0["mine"], r1["mine"])
    assert r0["reduced"].tobytes() == r1["reduced"].tobytes() == D.combine_actuator_stats([r0["mine"], r1["mine"]]).tobytes()


def test_the_carrier_state_goes_through_a_checkpoint_without_a_device(monkeypatch):
    """DeviceStats allocates a pinned buffer and an event at construction; with those two replaced the carrier runs on the CPU: its
    checkpoint members, and what loading them restores."""
    from kbot_joystick_amd.host import actuator as HA
    from kbot_joystick_amd.spec import compiler

    class NoEvent:
        def record(self): pass
        def synchronize(self): pass
    monkeypatch.setattr(torch.cuda, "Event", NoEvent)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    lv = HA.actuator_levels(compiler.load_model("kbot-headless"))
    a, b = HA.ActuatorStats(5, lv, "cpu"), HA.ActuatorStats(5, lv, "cpu")
    vec = AR.reference(*AR.SHAPES[3])[0][2]

    class FakeCtx:
        def actuator_stats(self, traj, levels, acc, stats, env=None):
            assert levels is lv
            acc += 1.0
            stats.copy_(torch.from_numpy(vec))
    for _ in range(2):
        a.after_rollout(FakeCtx(), None)
    last, total = a.vectors()
    assert last.tobytes() == vec.tobytes() and total.tobytes() == HA.dist_util.combine_actuator_stats([vec, vec]).tobytes()
    state = a.checkpoint_state()
    assert set(state) == {"act_acc", "act_total"} and state["act_acc"].shape == (5, A["SIZE"]) and (state["act_acc"] == 2.0).all()
    b.load_checkpoint_state(state)
    assert b.acc.numpy().tobytes() == a.acc.numpy().tobytes() and b.vectors()[1].tobytes() == total.tobytes() and not b.vectors()[0].any()
    b.load_checkpoint_state({"gait_acc": state["act_acc"]})               # a checkpoint without the members: from zero
    assert not b.acc.any() and not b.vectors()[1].any()
