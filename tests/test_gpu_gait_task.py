"""Gait statistics end to end through HumanoidWalkingTask: the gait/... scalars and totals against the host restatement on the task's own
trajectories, validation, the checkpoint members, off = off, and the gait sweep with its per-env record.

Bounds: the carry rows, the per-env record and every count, duration sum and maximum exact; the scalars are gait_scalars of a vector that
matches the restatement's at tests/gait_ref.assert_stats_match's bounds, so they are compared through the vectors."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import constants, layout as L
from tests import gait_ref as GR

pytestmark = pytest.mark.gpu
G, A, E, X, M = L.GAIT, L.GACC, L.GENV, L.AUX, L.CMODE


def _cfg(**kw):
    from kbot_joystick_amd.host.task import launch_config
    base = dict(num_envs=128, batch_size=64, hidden_size=64, num_passes=1, rollout_length_seconds=8 * 0.02, robot="kbot-headless", seed=5)
    base.update(kw)
    return launch_config(**base)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_scalars_totals_validation_and_checkpoint(tmp_path):
    """Every env is truncated after 5 steps, so with T = 8 episodes start inside every rollout and straddle the boundary."""
    from kbot_joystick_amd.host import dist as D
    from kbot_joystick_amd.host.gait import gait_scalars
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    cfg = _cfg(gait_stats=True, termination_params={"episode_length": {"max_length_sec": 5 * 0.02}})
    a = HumanoidWalkingTask(cfg)
    assert (a.T, a.N) == (8, 128) and a.gait is not None
    acc_ref, vectors = np.zeros((128, A["SIZE"]), np.float32), []
    for it in range(2):
        a.train_iteration()
        want, mags, _, _ = GR.gait_ref(acc_ref, a.traj.aux.cpu().numpy(), 8)
        last, total = a.gait_stats_vectors()
        vectors.append(last)
        GR.assert_stats_match(last, want, mags)
        assert want[G["EPISODES"]] >= 128 and np.array_equal(_bits(a.gait.acc.cpu().numpy()), _bits(acc_ref))
        assert total.tobytes() == D.combine_gait_stats(vectors).tobytes()                          # the totals are combine of the per-rollout vectors
        sc = a.scalars()
        gait = {k: v for k, v in sc.items() if k.startswith("gait/")}
        assert gait and gait == gait_scalars(last, cfg.ctrl_dt, "gait/") and "train/loss" in sc
        assert any(k.endswith("/double_support_frac") for k in gait) and any(k.endswith("/torque_rms") for k in gait)
    assert {k.replace("gait/", "gait_total/", 1) for k in gait} <= set(a.gait_stats(total=True))
    # validation: a fresh carry on the validation trajectory
    v = a.validate(num_envs=64, seconds=8 * 0.02)
    vg = {k: x for k, x in v.items() if k.startswith("valid/gait/")}
    want, mags, _, _ = GR.gait_ref(np.zeros((64, A["SIZE"]), np.float32), a._valid.traj.aux.cpu().numpy(), 8)
    ref_sc = gait_scalars(want, cfg.ctrl_dt, "valid/gait/")
    assert vg and set(vg) == set(ref_sc) and "valid/reward_per_step" in v
    for k, x in ref_sc.items():
        assert abs(vg[k] - x) <= 1e-9 * max(1.0, abs(x)), (k, vg[k], x)
    # checkpoint and resume: the carry rows, the totals and the next rollout's vector, bit for bit
    path = str(tmp_path / "ckpt.bin")
    a.save_checkpoint(path)
    b = HumanoidWalkingTask.load_task(path)
    assert b.config.gait_stats is True
    assert a.gait.acc.any() and a.gait.acc.cpu().numpy().tobytes() == b.gait.acc.cpu().numpy().tobytes()
    assert a.gait_stats_vectors()[1].tobytes() == b.gait_stats_vectors()[1].tobytes()
    a.train_iteration(); b.train_iteration()
    assert a.gait.acc.cpu().numpy().tobytes() == b.gait.acc.cpu().numpy().tobytes()
    for va, vb in zip(a.gait_stats_vectors(), b.gait_stats_vectors()):
        assert va.tobytes() == vb.tobytes()
    rows = lambda vec: sum(vec[L.gait_slot(m, "ROWS")] for m in range(M["COUNT"]))
    assert rows(a.gait_stats_vectors()[1]) == 3 * 8 * 128 and rows(a.gait_stats_vectors()[0]) == 8 * 128 and a.gait_stats() == b.gait_stats()
    a.close(); b.close()


def test_off_means_off():
    import dataclasses
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, HumanoidWalkingTaskConfig
    cfg_off = _cfg(deterministic=True, gait_stats=False)
    unmentioned = {k: v for k, v in dataclasses.asdict(cfg_off).items() if k != "gait_stats"}       # a task built without the field being mentioned
    unmentioned["action_latency_range"] = tuple(unmentioned["action_latency_range"])
    off, plain, on = HumanoidWalkingTask(cfg_off), HumanoidWalkingTask(HumanoidWalkingTaskConfig(**unmentioned)), HumanoidWalkingTask(_cfg(deterministic=True, gait_stats=True))
    assert off.gait is None and plain.gait is None
    for call in (off.gait_stats, off.gait_stats_vectors):
        with pytest.raises(B.KbjError, match="gait_stats=True"):
            call()
    for t in (off, plain, on):
        t.train_iteration()
    assert not any(k.startswith("gait/") for k in off.scalars()) and any(k.startswith("gait/") for k in on.scalars())
    extra = set(on.scalars()) - set(off.scalars())
    assert extra and all(k.startswith("gait/") for k in extra)
    assert not any(k.startswith("valid/gait/") for k in off.validate(num_envs=64, seconds=0.1))
    for other in (plain, on):          # the feature only observes: the iteration's outputs are the same bytes with the switch off, unmentioned, or on
        assert torch.equal(off.params, other.params) and torch.equal(off.opt_m, other.opt_m) and torch.equal(off.opt_v, other.opt_v)
        for name in ("actor_obs", "critic_obs", "aux", "action", "logp", "value", "reward", "adv", "target"):
            assert torch.equal(getattr(off.traj, name), getattr(other.traj, name)), name
    launches = []
    for task in (off, on):             # one more rollout under the library's kernel records: the switch adds one timed launch, off adds none
        task.ctx.profile_begin()
        task.rollout()
        launches.append({k["name"]: k["launches"] for k in task.ctx.profile_end()["kernels"]})
    assert launches[0] and not any("gait" in n for n in launches[0])
    assert launches[1] == dict(launches[0], **{"kbj::gait_stats_kernel": 1})
    for t in (off, plain, on):
        t.close()


def test_sweep_entries_are_pooled_from_the_per_env_record():
    """3 commands x 2 repeats, 1 s, freshly initialised parameters, every episode cut after 20 steps; the switch is off."""
    from kbot_joystick_amd.host import gait
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    task = HumanoidWalkingTask(_cfg(num_envs=64, termination_params={"episode_length": {"max_length_sec": 20 * 0.02}}))
    assert task.gait is None
    commands = [(0.6,), (0.0, 0.0, -0.5), ()]
    entries, rec = gait.gait_sweep(task, commands, repeats=2, seconds=1.0)
    T = 50
    aux, env = rec.aux.cpu().numpy(), rec.env.cpu().numpy()
    assert aux.shape == (T + 1, 6, X["SIZE"]) and env.shape == (6, E["SIZE"])
    want, mags, env_want, _ = GR.gait_ref(np.zeros((6, A["SIZE"]), np.float32), aux, T)
    assert np.array_equal(_bits(env), _bits(env_want))
    GR.assert_stats_match(rec.stats, want, mags)
    assert want[G["EPISODES"]] >= 12 and [e["mode"] for e in entries] == ["forward", "rotate", "stand"]
    done = aux[:T, :, X["DONE"]]
    for i, entry in enumerate(entries):
        envs = [i, i + 3]
        pooled = gait.pool_gait_rows(env_want[envs], task.config.ctrl_dt)
        assert entry["failures_per_s"] == float((done[:, envs] < 0).sum()) / (2 * T * task.config.ctrl_dt)
        for k, x in pooled.items():
            assert entry[k] == x or (x != x and entry[k] != entry[k]), (i, k, entry[k], x)
        assert abs(entry["double_support_frac"] + entry["single_support_frac"] + entry["flight_frac"] - 1.0) < 1e-12
        assert entry["torque_rms"] == np.sqrt(env_want[envs, G["TORQUE_SQ"]].astype(np.float64).sum() / (2 * T * L.NU))
    text = gait.format_gait_table(entries)
    assert len(text.splitlines()) == 4 and "xvel=+0.60" in text and "(zero)" in text
    print(text)
    assert len(task.gait_sweep(commands[:2], repeats=1, seconds=0.1)) == 2                       # the task's own entry point
    task.close()
