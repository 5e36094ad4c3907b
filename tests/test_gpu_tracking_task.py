"""Command-tracking errors end to end through HumanoidWalkingTask: the track/... scalars against the host restatement on the task's own
trajectories (fused and step-wise rollout, validation), the checkpoint members, off = off, and the sweep with its scripted commands.

Bounds: counts, fractions of counts and the carry rows exact; means, rms and maxima of an error within that error's row bound
max(4 S_k, 8 * 2^-24 M_k) worked out on the trajectory at hand (tests/tracking_ref.bounds_for) - a mean, an rms and a maximum of rows
move by no more than the rows do."""
import math

import numpy as np
import pytest

from kbot_joystick_amd.spec import constants, layout as L
from tests import tracking_ref as TR

pytestmark = pytest.mark.gpu
K, A, R, X = L.TRK, L.TACC, L.TERR, L.AUX
NE = L.NTERR


def _cfg(**kw):
    from kbot_joystick_amd.host.task import launch_config
    base = dict(num_envs=64, batch_size=64, hidden_size=64, num_passes=1, rollout_length_seconds=8 * 0.02, robot="kbot-headless", seed=5)
    base.update(kw)
    return launch_config(**base)


def _never(state, level):
    import torch
    return torch.zeros(state.N, device="cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _reference(task, aux, acc_ref, settle):
    jb = np.array(task.model_blob.joint_bias, np.float32)
    e64, bounds = TR.bounds_for(aux, jb, task.kcfg.rew_standard_height, task.kcfg.rew_foot_origin_height)
    want, _, rows = TR.tracking_ref(acc_ref, e64, aux, settle)
    return want, bounds, rows, e64


def _assert_scalars(got, want_vec, bounds, prefix):
    from kbot_joystick_amd.host.tracking import tracking_scalars
    want = tracking_scalars(want_vec, prefix)
    assert set(got) == set(want) and want, sorted(set(got) ^ set(want))
    for key, x in want.items():
        name = key.rsplit("/", 1)[1]
        if name in ("rows_frac", "settled_frac"):
            assert abs(got[key] - x) <= 1e-12, (key, got[key], x)
        else:
            k = constants.TRACKING_ERROR_NAMES.index(name.rsplit("_", 1)[0])
            assert abs(got[key] - x) <= bounds[k], (key, got[key], x, bounds[k])


def test_scalars_equal_the_reference_on_the_tasks_own_trajectories():
    """Every env is truncated after 5 steps, so with T = 8 episodes start inside every rollout and straddle the boundary; settle = 2 rows.
    The update is the deterministic one, so that the fused and the step-wise task hold the same parameters in the second rollout too."""
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    cfg = _cfg(deterministic=True, tracking_stats=True, tracking_settle_seconds=0.04, termination_params={"episode_length": {"max_length_sec": 5 * 0.02}})
    fused, step = HumanoidWalkingTask(cfg), HumanoidWalkingTask(cfg, extra_terminations={"never": _never})
    assert fused.tracking.settle_steps == 2 and (fused.T, fused.N) == (8, 64) and not fused.terms and step.terms
    acc_ref, totals = np.zeros((64, A["SIZE"]), np.float32), []
    for it in range(2):
        fused.train_iteration(); step.train_iteration()
        aux = fused.traj.aux.cpu().numpy()
        want, bounds, rows, _ = _reference(fused, aux[:8], acc_ref, 2)
        totals.append(want)
        assert 0 < rows[:, :, 1].sum() < rows[:, :, 1].size and want[K["EPISODES"]] >= 64
        last, total = fused.tracking_stats_vectors()
        counts = [m * K["MODE_STRIDE"] + s for m in range(L.CMODE["COUNT"]) for s in (K["ROWS"], K["SETTLED"])] + [K["CHANGES"], K["EPISODES"]]
        assert np.array_equal(last[counts], want[counts]) and np.array_equal(total[counts], sum(totals)[counts])
        assert np.array_equal(_bits(fused.tracking.acc.cpu().numpy()), _bits(acc_ref))
        sc = fused.scalars()
        track = {k: v for k, v in sc.items() if k.startswith("track/")}
        _assert_scalars(track, want, bounds, "track/")
        assert "train/loss" in sc
        assert {k: v for k, v in step.scalars().items() if k.startswith("track/")} == track        # the step-wise rollout: the same trajectory, the same bytes
        assert step.tracking_stats_vectors()[1].tobytes() == total.tobytes()
        if it == 1:
            assert {k.replace("track/", "track_total/", 1) for k in track} <= set(fused.tracking_stats(total=True))
    # validation: a fresh carry on the validation trajectory, on the fused and on the step-wise path
    v = fused.validate(num_envs=64, seconds=8 * 0.02)
    vt = {k: x for k, x in v.items() if k.startswith("valid/track/")}
    aux = fused._valid.traj.aux.cpu().numpy()
    want, bounds, _, _ = _reference(fused, aux[:8], np.zeros((64, A["SIZE"]), np.float32), 2)
    _assert_scalars(vt, want, bounds, "valid/track/")
    assert "valid/reward_per_step" in v
    assert fused.validate(num_envs=64, seconds=8 * 0.02, _stepwise=True) == v
    fused.close(); step.close()


def test_checkpoint_carries_the_tracking_state(tmp_path):
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    cfg = _cfg(tracking_stats=True, tracking_settle_seconds=0.04, termination_params={"episode_length": {"max_length_sec": 5 * 0.02}})
    a = HumanoidWalkingTask(cfg)
    for _ in range(2):
        a.train_iteration()
    path = str(tmp_path / "ckpt.bin")
    a.save_checkpoint(path)
    a.train_iteration()
    b = HumanoidWalkingTask.load_task(path)
    assert b.config.tracking_stats is True and b.config.tracking_settle_seconds == 0.04
    b.train_iteration()
    assert a.tracking.acc.any() and a.tracking.acc.cpu().numpy().tobytes() == b.tracking.acc.cpu().numpy().tobytes()
    for va, vb in zip(a.tracking_stats_vectors(), b.tracking_stats_vectors()):
        assert va.tobytes() == vb.tobytes()
    assert a.tracking_stats() == b.tracking_stats() and a.tracking_stats(total=True) == b.tracking_stats(total=True)
    rows = lambda v: sum(v[m * K["MODE_STRIDE"] + K["ROWS"]] for m in range(L.CMODE["COUNT"]))
    assert rows(a.tracking_stats_vectors()[1]) == 3 * 8 * 64 and rows(a.tracking_stats_vectors()[0]) == 8 * 64
    # a checkpoint of a run that did not keep the statistics loads into one that does: it starts from zero
    off = HumanoidWalkingTask(_cfg())
    off.train_iteration()
    path_off = str(tmp_path / "off.bin")
    off.save_checkpoint(path_off)
    b.load_checkpoint(path_off)
    assert not b.tracking.acc.any() and b.tracking_stats() == {} and rows(b.tracking_stats_vectors()[1]) == 0
    for t in (a, b, off):
        t.close()


def test_off_means_off():
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    off, on = HumanoidWalkingTask(_cfg(deterministic=True)), HumanoidWalkingTask(_cfg(deterministic=True, tracking_stats=True, tracking_settle_seconds=0.04))
    assert off.tracking is None
    with pytest.raises(B.KbjError, match="tracking_stats=True"):
        off.tracking_stats()
    for _ in range(2):
        off.train_iteration(); on.train_iteration()
    names = ("loss", "policy_loss", "value_loss", "entropy", "clip_fraction", "approx_kl", "adv_mean", "adv_std", "action_mirror_loss", "value_mirror_loss",
             "reward_per_step", "failures_per_step", "truncations_per_step", "value_mean", "action_std_logp")
    assert set(off.scalars()) == {f"train/{n}" for n in names}
    extra = set(on.scalars()) - set(off.scalars())
    assert extra and all(k.startswith("track/") for k in extra)
    assert not any(k.startswith("valid/track/") for k in off.validate(num_envs=64, seconds=0.1))
    assert any(k.startswith("valid/track/") for k in on.validate(num_envs=64, seconds=0.1))
    for name in ("actor_obs", "critic_obs", "aux", "action", "logp", "value", "reward", "adv", "target"):      # the feature only observes
        assert torch.equal(getattr(off.traj, name), getattr(on.traj, name)), name
    assert torch.equal(off.params, on.params) and torch.equal(off.opt_m, on.opt_m) and torch.equal(off.opt_v, on.opt_v)
    launches = []
    for task in (off, on):                      # a third rollout under the library's kernel records: the switch adds one timed launch, off adds none
        task.ctx.profile_begin()
        task.rollout()
        launches.append({k["name"]: k["launches"] for k in task.ctx.profile_end()["kernels"]})
    assert not any("tracking" in n for n in launches[0]) and launches[0]
    assert launches[1] == dict(launches[0], **{"kbj::tracking_stats_kernel": 1})
    off.close(); on.close()


def test_sweep_holds_every_command_through_resets():
    """6 commands x 2 repeats, 100 steps, freshly initialised parameters, every episode cut after 40 steps: each env is reset twice, and the
    kernel's reset returns it to the context's fixed (zero) command - the scripted term must hand it its own again."""
    from kbot_joystick_amd.host import tracking
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    task = HumanoidWalkingTask(_cfg(termination_params={"episode_length": {"max_length_sec": 40 * 0.02}}))
    commands = [(0.6,), (0.0, 0.3), (0.0, 0.0, -0.5), (0.4, 0.2, 0.3, 0, 0, 0, 0.3), (0, 0, 0, -0.1, 0.1, -0.1), ()]
    entries, rec = tracking.tracking_sweep(task, commands, repeats=2, seconds=100 * 0.02, settle_seconds=0.2)
    assert len(entries) == 6 and [e["mode"] for e in entries] == list(constants.COMMAND_MODE_NAMES)
    aux, err = rec.aux.cpu().numpy(), rec.err.cpu().numpy()
    assert aux.shape == (101, 12, X["SIZE"]) and err.shape == (100, 12, R["SIZE"])
    table = np.zeros((6, L.NCMD), np.float32)
    for i, c in enumerate(commands):
        table[i, :len(c)] = c
    assert np.array_equal(aux[:, :, X["CMD"]:X["CMD"] + L.NCMD], np.broadcast_to(np.tile(table, (2, 1)), (101, 12, L.NCMD)))       # every row, behind every reset
    done = aux[:100, :, X["DONE"]]
    assert (done != 0).any(axis=0).all(), "no env was reset: the test shows nothing about commands surviving one"
    want, bounds, rows, e64 = _reference(task, aux[:100], np.zeros((12, A["SIZE"]), np.float32), 10)
    assert np.array_equal(err[:, :, R["SETTLED"]], rows[:, :, 1]) and np.array_equal(err[:, :, R["SINCE"]], rows[:, :, 2]) and np.array_equal(err[:, :, R["MODE"]], rows[:, :, 0])
    assert want[K["CHANGES"]] == 0 and rec.stats[K["CHANGES"]] == 0 and rec.stats[K["EPISODES"]] == want[K["EPISODES"]] >= 36
    settled = rows[:, :, 1] != 0
    assert settled.any()
    for i, entry in enumerate(entries):
        envs = (i, i + 6)
        assert entry["command"] == tuple(float(x) for x in table[i])
        assert entry["settled_rows"] == int(settled[:, envs].sum())
        assert entry["failures_per_s"] == float((done[:, envs] < 0).sum()) / (2 * 100 * task.config.ctrl_dt)
        for k, name in enumerate(constants.TRACKING_ERROR_NAMES):
            means = [e64[settled[:, j], j, k].mean() for j in envs if settled[:, j].any()]       # per env over its settled rows, then over the repeats
            assert (math.isnan(entry[name]) and not means) or abs(entry[name] - np.mean(means)) <= bounds[k], (i, name, entry[name], means, bounds[k])
    text = tracking.format_tracking_table(entries)
    assert len(text.splitlines()) == 7 and "xvel=+0.60" in text and "(zero)" in text
    print(text)
    # the task's own entry point, the default grid, a run too short for anything to settle: no mean to report
    short = task.tracking_sweep(repeats=4, seconds=5 * 0.02)
    assert len(short) == 15 and all(e["settled_rows"] == 0 and math.isnan(e["lin_vel_err"]) for e in short)
    assert sum(e["mode"] == "forward" for e in short) == 4 and short[0]["mode"] == "stand"
    task.close()
