"""Actuator statistics end to end through HumanoidWalkingTask: the act/... scalars and totals against the host restatement on the task's own
trajectories, validation, the checkpoint members, off = off, the actuator sweep with its per-env record, and the gait sweep untouched by the
sweeps' new record_state argument.

Bounds: the carry rows, the per-env record and every count and maximum exact; the scalars are actuator_scalars of a vector that matches the
restatement's at tests/actuator_ref.assert_stats_match's bounds, so they are compared through the vectors."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import actuator_ref as AR

pytestmark = pytest.mark.gpu
V, A, E, X, Q, M = L.ACT, L.AACC, L.AENV, L.AUX, L.QSTATE, L.CMODE


def _cfg(**kw):
    from kbot_joystick_amd.host.task import launch_config
    base = dict(num_envs=64, batch_size=64, hidden_size=64, num_passes=1, rollout_length_seconds=8 * 0.02, robot="kbot-headless", seed=5)
    base.update(kw)
    return launch_config(**base)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rows(task_traj):
    return task_traj.aux.cpu().numpy(), task_traj.qstate.cpu().numpy(), task_traj.action.cpu().numpy()


def test_scalars_totals_validation_and_checkpoint(tmp_path):
    """Every env is truncated after 5 steps, so with T = 8 episodes start inside every rollout and straddle the boundary."""
    from kbot_joystick_amd.host import dist as D
    from kbot_joystick_amd.host.actuator import actuator_scalars
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    cfg = _cfg(actuator_stats=True, record_state=True, actuator_torque_level=0.5, termination_params={"episode_length": {"max_length_sec": 5 * 0.02}})
    a = HumanoidWalkingTask(cfg)
    assert (a.T, a.N) == (8, 64) and a.actuator is not None and a.actuator.levels.tau_level[3] == 42.0
    lvd = AR.levels_dict(a.actuator.levels)
    acc_ref, vectors = np.zeros((64, A["SIZE"]), np.float32), []
    for it in range(2):
        a.train_iteration()
        want, mags, _ = AR.actuator_ref(acc_ref, *_rows(a.traj), 8, lvd)
        last, total = a.actuator_stats_vectors()
        vectors.append(last)
        AR.assert_stats_match(last, want, mags)
        assert want[V["EPISODES"]] >= 64 and np.array_equal(_bits(a.actuator.acc.cpu().numpy()), _bits(acc_ref))
        assert total.tobytes() == D.combine_actuator_stats(vectors).tobytes()                      # the totals are combine of the per-rollout vectors
        sc = a.scalars()
        act = {k: v for k, v in sc.items() if k.startswith("act/")}
        ref_sc = actuator_scalars(last, a.model_blob, cfg.ctrl_dt, "act/", a.actuator.levels)
        assert act and set(act) == set(ref_sc) and all(act[k] == x or (x != x and act[k] != act[k]) for k, x in ref_sc.items()) and "train/loss" in sc
        assert any(k.endswith("/power_abs_w") for k in act) and any(k.endswith("/worst_joint_frac") for k in act) and len(act) <= 10 * M["COUNT"]
    assert {k.replace("act/", "act_total/", 1) for k in act} <= set(a.actuator_stats(total=True))
    table = a.actuator_stats(per_joint=True)
    assert len(table) == L.NU and table[3]["joint"] == "dof_left_knee_04" and table[3]["torque_max_frac"] > 0
    # validation: a fresh carry on the validation trajectory, which keeps its state record when the switch is on
    v = a.validate(num_envs=64, seconds=8 * 0.02)
    vg = {k: x for k, x in v.items() if k.startswith("valid/act/")}
    want, mags, _ = AR.actuator_ref(np.zeros((64, A["SIZE"]), np.float32), *_rows(a._valid.traj), 8, lvd)
    ref_sc = actuator_scalars(want, a.model_blob, cfg.ctrl_dt, "valid/act/", a.actuator.levels)
    assert vg and set(vg) == set(ref_sc) and "valid/reward_per_step" in v
    for k, x in ref_sc.items():
        assert abs(vg[k] - x) <= 1e-9 * max(1.0, abs(x)) or (x != x and vg[k] != vg[k]), (k, vg[k], x)
    # checkpoint and resume: the carry rows, the totals and the next rollout's vector, bit for bit
    path = str(tmp_path / "ckpt.bin")
    a.save_checkpoint(path)
    b = HumanoidWalkingTask.load_task(path)
    assert b.config.actuator_stats is True and b.config.record_state is True and b.config.actuator_torque_level == 0.5
    assert a.actuator.acc.any() and a.actuator.acc.cpu().numpy().tobytes() == b.actuator.acc.cpu().numpy().tobytes()
    assert a.actuator_stats_vectors()[1].tobytes() == b.actuator_stats_vectors()[1].tobytes()
    a.train_iteration(); b.train_iteration()
    assert a.actuator.acc.cpu().numpy().tobytes() == b.actuator.acc.cpu().numpy().tobytes()
    for va, vb in zip(a.actuator_stats_vectors(), b.actuator_stats_vectors()):
        assert va.tobytes() == vb.tobytes()
    rows = lambda vec: sum(vec[L.act_slot(m, "ROWS")] for m in range(M["COUNT"]))
    assert rows(a.actuator_stats_vectors()[1]) == 3 * 8 * 64 and rows(a.actuator_stats_vectors()[0]) == 8 * 64
    a.close(); b.close()


def test_off_means_off():
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    off, on = HumanoidWalkingTask(_cfg(deterministic=True, record_state=True)), HumanoidWalkingTask(_cfg(deterministic=True, record_state=True, actuator_stats=True))
    assert off.actuator is None and off.config.actuator_stats is False
    for call in (off.actuator_stats, off.actuator_stats_vectors):
        with pytest.raises(B.KbjError, match="actuator_stats=True"):
            call()
    for t in (off, on):
        t.train_iteration()
    assert not any(k.startswith("act/") for k in off.scalars()) and any(k.startswith("act/") for k in on.scalars())
    extra = set(on.scalars()) - set(off.scalars())
    assert extra and all(k.startswith("act/") for k in extra)
    assert not any(k.startswith("valid/act/") for k in off.validate(num_envs=64, seconds=0.1))
    assert torch.equal(off.params, on.params) and torch.equal(off.opt_m, on.opt_m)          # the feature only observes
    for name in ("actor_obs", "critic_obs", "aux", "action", "logp", "value", "reward", "adv", "target", "qstate"):
        assert torch.equal(getattr(off.traj, name), getattr(on.traj, name)), name
    launches = []
    for task in (off, on):             # one more rollout under the library's kernel records: the switch adds its two launches, off adds none
        task.ctx.profile_begin()
        task.rollout()
        launches.append({k["name"]: k["launches"] for k in task.ctx.profile_end()["kernels"]})
    assert launches[0] and not any("actuator" in n or "ActSlots" in n for n in launches[0])
    assert launches[1] == dict(launches[0], **{"kbj::actuator_stats_kernel": 1, "kbj::ordered_reduce_wide_kernel<kbj::ActSlots>": 1})
    for t in (off, on):
        t.close()


def test_sweep_entries_are_pooled_from_the_per_env_record_and_the_gait_sweep_is_as_before(monkeypatch):
    """2 commands x 2 repeats, 1 s, freshly initialised parameters, every episode cut after 20 steps; both switches are off."""
    from kbot_joystick_amd.host import actuator, gait, sweep
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    task = HumanoidWalkingTask(_cfg(termination_params={"episode_length": {"max_length_sec": 20 * 0.02}}))
    assert task.actuator is None and task.config.record_state is False
    commands = [(0.6,), ()]
    entries, rec = actuator.actuator_sweep(task, commands, repeats=2, seconds=1.0, torque_level=0.5, speed_limit=4.0)
    T = 50
    aux, qs, act, env = rec.aux.cpu().numpy(), rec.qstate.cpu().numpy(), rec.action.cpu().numpy(), rec.env.cpu().numpy()
    assert aux.shape == (T + 1, 4, X["SIZE"]) and qs.shape == (T, 4, Q["SIZE"]) and env.shape == (4, E["SIZE"]) and rec.levels.tau_level[3] == 42.0 and rec.levels.vel_level[0] == 4.0
    want, mags, env_want = AR.actuator_ref(np.zeros((4, A["SIZE"]), np.float32), aux, qs, act, T, AR.levels_dict(rec.levels))
    assert np.array_equal(_bits(env), _bits(env_want))
    AR.assert_stats_match(rec.stats, want, mags)
    assert want[V["EPISODES"]] >= 8 and [e["mode"] for e in entries] == ["forward", "stand"]
    done = aux[:T, :, X["DONE"]]
    for i, entry in enumerate(entries):
        envs = [i, i + 2]
        pooled = actuator.pool_actuator_rows(env_want[envs], task.model_blob, task.config.ctrl_dt)
        assert entry["failures_per_s"] == float((done[:, envs] < 0).sum()) / (2 * T * task.config.ctrl_dt)
        for k, x in pooled.items():
            assert entry[k] == x or (x != x and entry[k] != entry[k]), (i, k, entry[k], x)
        assert entry["torque_rms"] == np.sqrt(env_want[envs, E["TAU_SQ"]].astype(np.float64).sum() / (2 * T * L.NU)) and entry["power_abs_w"] > 0
    text = actuator.format_actuator_table(entries)
    assert len(text.splitlines()) == 3 and "xvel=+0.60" in text and "(zero)" in text and "dof_" in text
    print(text)
    assert len(task.actuator_sweep(commands[:1], repeats=1, seconds=0.1)) == 1                     # the task's own entry point, the config's levels
    # the gait sweep does not pass record_state: it returns what a call that passes the default explicitly returns, and keeps no state record
    first, rec_first = gait.gait_sweep(task, commands, repeats=2, seconds=0.5)
    seen, held_command_rollout = [], sweep.held_command_rollout

    def explicit(task_, n, T_, command, seed_offset, record_state=None):
        seen.append(record_state)
        return held_command_rollout(task_, n, T_, command, seed_offset, record_state=False)
    monkeypatch.setattr(sweep, "held_command_rollout", explicit)      # where the command sweeps' rollout is started from
    second, rec_second = gait.gait_sweep(task, commands, repeats=2, seconds=0.5)
    assert seen == [None] and repr(first) == repr(second) and rec_first.stats.tobytes() == rec_second.stats.tobytes()
    assert rec_first.aux.cpu().numpy().tobytes() == rec_second.aux.cpu().numpy().tobytes() and rec_first.env.cpu().numpy().tobytes() == rec_second.env.cpu().numpy().tobytes()
    task.close()
