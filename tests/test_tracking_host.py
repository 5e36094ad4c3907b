"""Command-tracking errors, the parts that need no GPU: the layout mirrors, the mode rule, the settle scan pinned on a hand-computed case, the
scalars, combining vectors, the config fields and checkpoint members, the default grid and the table - and the conditions the synthetic
problems of tests/test_gpu_tracking_stats.py must meet for that test to mean something, with the float32-against-float64 spread its
error bounds are built from."""
import dataclasses

import numpy as np

from kbot_joystick_amd.spec import constants, layout as L
from tests import tracking_ref as TR

K, A, R, X, M = L.TRK, L.TACC, L.TERR, L.AUX, L.CMODE


def test_layout_mirrors_the_header():
    assert L.NTERR == len(constants.TRACKING_ERROR_NAMES)                                     # (values against the header: tests/test_abi_mirror.py)
    assert constants.COMMAND_MODE_NAMES == ("forward", "sideways", "rotate", "omni", "stand_bend", "stand")      # the switch list of train.py:752-762
    assert [M[n.upper()] for n in constants.COMMAND_MODE_NAMES] == list(range(M["COUNT"]))
    assert M["COUNT"] * K["MODE_STRIDE"] == K["CHANGES"] and K["MAX"] + L.NTERR <= K["MODE_STRIDE"] and K["EPISODES"] < K["SIZE"]
    assert A["CMD"] + L.NCMD == A["SINCE"] and A["RUNNING"] < A["SIZE"] and A["SIZE"] % 4 == 0


def test_modes_of_the_prototype_commands():
    """The six prototype vectors of train.py:744-749 classify as their own mode; moving commands with arms are omni; -0.0 counts as zero."""
    from kbot_joystick_amd.host.tracking import command_mode
    vx, vy, wz, bh, rx, ry = 0.7, -0.3, 0.5, -0.1, 0.2, -0.2
    arms = [0.0, 0.3, 0.0, -0.2, 0.0, 0.0, 0.1, 0.0, 0.0, 0.4]
    z, zz = [0.0], [0.0] * 10
    protos = [[vx] + z * 5 + zz, z + [vy] + z * 4 + zz, z * 2 + [wz] + z * 3 + zz, [vx, vy, wz] + z * 3 + arms, z * 3 + [bh, rx, ry] + arms, z * 6 + zz]
    for mode, cmd in enumerate(protos):
        assert len(cmd) == L.NCMD
        for f in (TR.mode_of, command_mode):
            assert f(np.array(cmd, np.float32)) == mode, (mode, cmd)
    for f in (TR.mode_of, command_mode):
        assert f(np.array([vx] + z * 5 + arms, np.float32)) == M["OMNI"]                      # forward with arms
        assert f(np.array(z * 2 + [wz] + [bh] + z * 2 + zz, np.float32)) == M["OMNI"]          # turning with a height command
        assert f(np.array([vx, vy] + z * 4 + zz, np.float32)) == M["OMNI"]                     # two velocities, no pose
        assert f(np.array(z * 6 + [0.0] * 9 + [1e-30], np.float32)) == M["STAND_BEND"]         # exact != 0 tests
        neg = np.array([vx] + [-0.0] * 15, np.float32)
        assert np.signbit(neg[1]) and f(neg) == M["FORWARD"]
        assert f(np.array([-0.0] * 16, np.float32)) == M["STAND"]


def test_hand_computed_scan():
    """T = 3, N = 1, settle_steps = 1, a fresh carry. Row 0 starts an episode (since 0: transient). Row 1 changes the command from forward to
    sideways (since 0: transient, a change) and ends the episode. Row 2 starts the next episode with the same command (since 0: transient, no
    change counted). Then a second call of the same three rows against the carry: row 0 compares with the carried sideways command of a
    RUNNING episode -> a change; and with settle_steps = 0 everything is settled."""
    aux = np.zeros((3, 1, X["SIZE"]), np.float32)
    aux[0, 0, X["CMD"]] = 0.5
    aux[1:, 0, X["CMD"] + 1] = 0.25
    aux[1, 0, X["DONE"]] = -1
    err = np.zeros((3, 1, L.NTERR), np.float32)
    err[:, 0, 0], err[:, 0, 4] = (1.0, 2.0, 4.0), (0.5, 0.25, 8.0)
    acc = np.zeros((1, A["SIZE"]), np.float32)
    acc[0, 18:] = 7.0
    st, _, rows = TR.tracking_ref(acc, err, aux, 1)
    assert rows[:, 0].tolist() == [[M["FORWARD"], 0, 0], [M["SIDEWAYS"], 0, 0], [M["SIDEWAYS"], 0, 0]]
    assert (st[K["CHANGES"]], st[K["EPISODES"]]) == (1, 2)
    fwd, side = M["FORWARD"] * K["MODE_STRIDE"], M["SIDEWAYS"] * K["MODE_STRIDE"]
    assert (st[fwd + K["ROWS"]], st[side + K["ROWS"]], st[fwd + K["SETTLED"]], st[side + K["SETTLED"]]) == (1, 2, 0, 0)
    assert st.sum() == 3 + 3                                                  # nothing else: no settled row, no sum
    assert acc[0, A["CMD"] + 1] == 0.25 and acc[0, A["CMD"]] == 0 and (acc[0, A["SINCE"]], acc[0, A["RUNNING"]]) == (0, 1) and (acc[0, 18:] == 7).all()
    # the second call: row 0 changes the command of the running episode; row 2 follows row 1's DONE again
    st, _, rows = TR.tracking_ref(acc, err, aux, 1)
    assert rows[:, 0, 2].tolist() == [0, 0, 0] and (st[K["CHANGES"]], st[K["EPISODES"]]) == (2, 1)
    # three rows of one command, no DONE: since 0, 1, 2; settle_steps = 1 counts the last two
    aux[:, 0, X["CMD"]:X["CMD"] + 2], aux[:, 0, X["DONE"]] = (0.5, 0.0), 0
    acc[:] = 0
    st, mags, rows = TR.tracking_ref(acc, err, aux, 1)
    assert rows[:, 0, 2].tolist() == [0, 1, 2] and rows[:, 0, 1].tolist() == [0, 1, 1]
    assert (st[fwd + K["ROWS"]], st[fwd + K["SETTLED"]], st[fwd + K["SUM"]], st[fwd + K["SUMSQ"]], st[fwd + K["MAX"]]) == (3, 2, 6.0, 20.0, 4.0)
    assert (st[fwd + K["SUM"] + 4], st[fwd + K["SUMSQ"] + 4], st[fwd + K["MAX"] + 4]) == (8.25, 64.0625, 8.0) and mags[fwd + K["SUM"]] == 6.0
    assert (acc[0, A["SINCE"]], acc[0, A["RUNNING"]]) == (2, 1)
    st, _, rows = TR.tracking_ref(acc, err, aux, 0)                           # carried on: since 3, 4, 5, all settled
    assert rows[:, 0, 2].tolist() == [3, 4, 5] and st[fwd + K["SETTLED"]] == 3 and (st[K["CHANGES"]], st[K["EPISODES"]]) == (0, 0)


def test_errors_of_a_hand_computed_row():
    """Base yawed by 90 degrees, commanded 1 m/s forward, moving 0.6 m/s along world y: 0.4 m/s off. Level base against a commanded roll of 0.2 rad:
    1 - cos^2(0.1). Base 0.9 m over feet at 0.05 / 0.07 m with a -0.1 m height command: |0.9 - (0.05 - 0.06) - 0.7| = 0.21."""
    a = np.zeros((1, X["SIZE"]), np.float32)
    a[0, X["BQUAT"]:X["BQUAT"] + 4] = (np.cos(np.pi / 4), 0, 0, np.sin(np.pi / 4))
    a[0, X["QVEL"] + 1], a[0, X["QVEL"] + 5] = 0.6, 0.3
    a[0, X["CMD"]], a[0, X["CMD"] + 2], a[0, X["CMD"] + 3], a[0, X["CMD"] + 4] = 1.0, -0.2, -0.1, 0.2
    a[0, X["BASEZ"]], a[0, X["LFZ"]], a[0, X["RFZ"]] = 0.9, 0.05, 0.07
    jb = TR.joint_bias()
    a[0, X["ARMQ"]:X["ARMQ"] + 10] = jb[10:]
    a[0, X["ARMQ"] + 3] += 0.5
    for dtype, tol in ((np.float64, 5e-7), (np.float32, 2e-6)):       # the inputs are float32 roundings of the decimals (2^-24 of values up to 2)
        e, mag = TR.errors(a, jb, 0.8, 0.06, dtype)
        want = (0.4, 0.5, 1 - np.cos(0.1) ** 2, 0.21, 0.25)
        assert np.abs(e[0] - want).max() < tol, (dtype, e[0], want)
        assert mag[2] == 1.0 and abs(mag[0] - 1.0) < 1e-6


def test_scalars_omit_modes_without_settled_rows():
    from kbot_joystick_amd.host import dist as D
    from kbot_joystick_amd.host.tracking import tracking_scalars
    assert tracking_scalars(D.empty_tracking_stats()) == {}
    v = D.empty_tracking_stats()
    fwd, stand = M["FORWARD"] * K["MODE_STRIDE"], M["STAND"] * K["MODE_STRIDE"]
    v[fwd + K["ROWS"]], v[fwd + K["SETTLED"]], v[fwd + K["SUM"]], v[fwd + K["SUMSQ"]], v[fwd + K["MAX"]] = 6, 4, 2.0, 1.44, 0.9
    v[fwd + K["SUM"] + 3], v[fwd + K["SUMSQ"] + 3], v[fwd + K["MAX"] + 3] = 0.4, 0.08, 0.2
    v[stand + K["ROWS"]] = 2                                                  # rows, none settled: omitted
    s = tracking_scalars(v, "x/")
    want = {"x/forward/lin_vel_err_mean": 0.5, "x/forward/lin_vel_err_rms": 0.6, "x/forward/lin_vel_err_max": 0.9, "x/forward/height_err_mean": 0.1,
            "x/forward/height_err_rms": 0.02 ** 0.5, "x/forward/height_err_max": 0.2, "x/forward/rows_frac": 0.75, "x/forward/settled_frac": 4 / 6}
    for k, x in want.items():
        assert abs(s[k] - x) < 1e-12, (k, s[k], x)
    assert set(s) == {f"x/forward/{e}_{q}" for e in constants.TRACKING_ERROR_NAMES for q in ("mean", "rms", "max")} | {"x/forward/rows_frac", "x/forward/settled_frac"}
    assert s["x/forward/yaw_rate_err_mean"] == 0.0 and not any("stand" in k for k in s)


def _three_vectors():
    out = []
    for T, N in TR.SHAPES[1:]:
        aux = TR.problems(T, N).calls[0]
        e32 = TR.spread()[2][(T, N, 0)][1]
        out.append(TR.tracking_ref(np.zeros((N, A["SIZE"]), np.float32), e32, aux, 1)[0])
    return out


def test_combine_is_associative_with_the_empty_vector_as_identity():
    from kbot_joystick_amd.host import dist as D
    a, b, c = _three_vectors()
    assert all(v[M["OMNI"] * K["MODE_STRIDE"] + K["SETTLED"]] > 0 for v in (a, b, c))
    e = D.empty_tracking_stats()
    assert np.array_equal(D.combine_tracking_stats([]), e) and np.array_equal(D.combine_tracking_stats([a, e]), a) and np.array_equal(D.combine_tracking_stats([e, a]), a)
    left, right = D.combine_tracking_stats([D.combine_tracking_stats([a, b]), c]), D.combine_tracking_stats([a, D.combine_tracking_stats([b, c])])
    hi = np.zeros(K["SIZE"], bool)
    hi[D.TRACKING_STATS.hi] = True
    assert hi.sum() == M["COUNT"] * L.NTERR
    assert np.array_equal(left[hi], right[hi]) and np.array_equal(left[hi], np.maximum(np.maximum(a, b), c)[hi])
    assert np.allclose(left, right, rtol=1e-15, atol=0) and np.allclose(left[~hi], (a + b + c)[~hi], rtol=1e-15, atol=0)     # float64 adds: associative to a rounding
    counts = [m * K["MODE_STRIDE"] + s for m in range(M["COUNT"]) for s in (K["ROWS"], K["SETTLED"])] + [K["CHANGES"], K["EPISODES"]]
    assert np.array_equal(left[counts], right[counts]) and np.array_equal(left[counts], (a + b + c)[counts])
    # halves of the envs of one problem make the whole
    T, N = TR.SHAPES[2]
    aux, e32 = TR.problems(T, N).calls[0], TR.spread()[2][(T, N, 0)][1]
    whole, mags, _ = TR.tracking_ref(np.zeros((N, A["SIZE"]), np.float32), e32, aux, 1)
    halves = [TR.tracking_ref(np.zeros((N // 2, A["SIZE"]), np.float32), e32[:, s], aux[:, s], 1)[0] for s in (slice(0, N // 2), slice(N // 2, N))]
    TR.assert_stats_match(D.combine_tracking_stats(halves), whole, mags)
    import torch
    assert np.array_equal(D.reduce_tracking_stats(torch.from_numpy(whole), 1).numpy(), whole)       # one rank: no collective


def test_the_synthetic_problems_exercise_what_the_gpu_test_claims():
    """Conditions, not tolerances, checked on the reference alone, over the problems of all shapes together: every mode occurs; at
    settle_steps = 3 settled and transient rows are each at least 10 % of the rows; no base quaternion is near the asin clamp
    (|2 (wy - zx)| <= 0.9); no |cmd[0:3]| lies within 1e-4 of the rewards' zero-command threshold 1e-3. Prints the spread S_k."""
    S, mag, per = TR.spread()
    bounds = TR.error_bounds()
    for k, name in enumerate(constants.TRACKING_ERROR_NAMES):
        print(f"{name}: float32-against-float64 spread S = {S[k]:.3e}, largest operand M = {mag[k]:.3e}, bound max(4 S, 8 * 2^-24 M) = {bounds[k]:.3e}")
    assert (S > 0).all() and (S < 1e-5).all() and (bounds < 5e-5).all()
    rows_mode, settled, total, changes, episodes, negzero = np.zeros(M["COUNT"]), 0, 0, 0, 0, 0
    for T, N in TR.SHAPES:
        acc = np.zeros((N, A["SIZE"]), np.float32)
        P = TR.problems(T, N)
        for call, aux in enumerate(P.calls):
            st, _, rows = TR.tracking_ref(acc, per[(T, N, call)][1], aux, 3)
            rows_mode += [st[m * K["MODE_STRIDE"] + K["ROWS"]] for m in range(M["COUNT"])]
            settled += rows[:, :, 1].sum(); total += T * N
            changes += st[K["CHANGES"]]; episodes += st[K["EPISODES"]]
            w, x, y, z = (aux[:T, :, X["BQUAT"] + k].astype(np.float64) for k in range(4))
            assert np.abs(2 * (w * y - z * x)).max() <= 0.9
            c = aux[:T, :, X["CMD"]:X["CMD"] + 3].astype(np.float64)
            assert (np.abs(np.sqrt((c * c).sum(-1)) - 1e-3) > 1e-4).all()
            cmd = aux[:T, :, X["CMD"]:X["CMD"] + L.NCMD]
            negzero += int((np.signbit(cmd) & (cmd == 0)).sum())
            if N >= 4:
                assert (rows[:, 1, 2] == np.arange(call * T, call * T + T)).all()       # env 1: one command, one episode, SINCE through the calls
                assert rows[0, 0, 2] == 0 and aux[T - 1, N - 1, X["DONE"]] != 0
                if T >= 3:
                    assert aux[1, 2, X["DONE"]] != 0 and aux[2, 2, X["DONE"]] != 0 and rows[2, 2, 2] == 0
    assert (rows_mode > 0).all(), rows_mode
    assert 0.1 * total <= settled <= 0.9 * total, (settled, total)
    assert changes > 0 and episodes > 0 and negzero > 0


def test_config_fields_and_checkpoint_members(tmp_path, monkeypatch):
    from kbot_joystick_amd.host import ckpt, dist as D
    from kbot_joystick_amd.host.task import HumanoidWalkingTaskConfig, launch_config
    from kbot_joystick_amd.host.tracking import settle_steps
    monkeypatch.delenv("KBJ_TRACKING_STATS", raising=False)
    assert HumanoidWalkingTaskConfig().tracking_stats is False and launch_config().tracking_stats is False and launch_config().tracking_settle_seconds == 0.5
    monkeypatch.setenv("KBJ_TRACKING_STATS", "1")
    assert HumanoidWalkingTaskConfig().tracking_stats is True and HumanoidWalkingTaskConfig(tracking_stats=False).tracking_stats is False
    monkeypatch.setenv("KBJ_TRACKING_STATS", "0")
    assert HumanoidWalkingTaskConfig().tracking_stats is False
    assert (settle_steps(0.5, 0.02), settle_steps(0.0, 0.02), settle_steps(0.07, 0.02)) == (25, 0, 4)
    cfg = launch_config(tracking_stats=True, tracking_settle_seconds=0.1, hidden_size=16, depth=1)
    d = dataclasses.asdict(cfg)
    assert d["tracking_stats"] is True and d["tracking_settle_seconds"] == 0.1
    d["action_latency_range"] = tuple(d["action_latency_range"])
    assert HumanoidWalkingTaskConfig(**d) == cfg
    old = {k: v for k, v in d.items() if not k.startswith("tracking_")}              # a config member written before the fields existed
    assert HumanoidWalkingTaskConfig(**old).tracking_stats is False
    P = sum(L.param_count(16, 1))
    p = np.arange(P, dtype=np.float32)
    d["action_latency_range"] = list(d["action_latency_range"])
    acc = np.random.default_rng(0).uniform(0, 9, (4, A["SIZE"])).astype(np.float32)
    total = D.empty_tracking_stats()
    total[K["ROWS"]], total[K["SUM"]] = 7, 0.1 + 0.2
    without, with_ = str(tmp_path / "old.bin"), str(tmp_path / "new.bin")
    ckpt.save_ckpt(without, p, p, p, 1, 16, 1, dict(num_steps=1), d, dict(es=np.zeros((4, L.ES["SIZE"]), np.float32)))
    ckpt.save_ckpt(with_, p, p, p, 1, 16, 1, dict(num_steps=1), d, dict(es=np.zeros((4, L.ES["SIZE"]), np.float32), trk_acc=acc, trk_total=total))
    x = ckpt.load_ckpt(without, "all")["extras"]
    assert "trk_acc" not in x and "trk_total" not in x and "es" in x
    z = ckpt.load_ckpt(with_, "all")
    assert z["config"]["tracking_stats"] is True and z["config"]["tracking_settle_seconds"] == 0.1
    assert z["extras"]["trk_acc"].dtype == np.float32 and np.array_equal(z["extras"]["trk_acc"], acc)
    assert z["extras"]["trk_total"].dtype == np.float64 and np.array_equal(z["extras"]["trk_total"], total)


def test_default_grid_and_table():
    from kbot_joystick_amd.host.tracking import command_mode, default_command_grid, format_tracking_table
    from kbot_joystick_amd.host.task import launch_config
    kcfg = launch_config(command_ranges={"vx_range": (-0.25, 1.0)}).to_kbj(4096)
    grid = default_command_grid(kcfg)
    assert len(grid) == 15 and all(len(c) == L.NCMD for c in grid) and len(set(grid)) == 15
    modes = [command_mode(c) for c in grid]
    assert modes[0] == M["STAND"] and modes[-2:] == [M["OMNI"], M["STAND_BEND"]]
    assert modes[1:13] == [M["FORWARD"]] * 4 + [M["SIDEWAYS"]] * 4 + [M["ROTATE"]] * 4
    assert [c[0] for c in grid[1:5]] == [0.5, 1.0, -0.125, -0.25]                               # half and full of the configured range, both directions
    assert [c[1] for c in grid[5:9]] == [0.25, 0.5, -0.25, -0.5] and [c[2] for c in grid[9:13]] == [0.5, 1.0, -0.5, -1.0]
    entries = [dict(command=grid[2], mode="forward", lin_vel_err=0.18, yaw_rate_err=0.05, tilt_err=0.001, height_err=0.02, arm_sq_err=0.3, settled_rows=950, failures_per_s=0.1),
               dict(command=grid[0], mode="stand", lin_vel_err=0.03, yaw_rate_err=0.01, tilt_err=0.0, height_err=0.01, arm_sq_err=0.1, settled_rows=0, failures_per_s=0.0)]
    text = format_tracking_table(entries).splitlines()
    assert len(text) == 3 and all(n in text[0] for n in constants.TRACKING_ERROR_NAMES) and "settled" in text[0]
    assert text[1].startswith("xvel=+1.00") and "forward" in text[1] and "0.1800" in text[1] and "950" in text[1]
    assert text[2].startswith("(zero)") and "stand" in text[2]
