"""The four statistics the device keeps over the rollouts - episodes, tracking, gait, actuator - switched on TOGETHER in one
HumanoidWalkingTask: every group of scalars() is its module's scalars function of the task's own vector, validate() carries all four groups,
and a checkpoint takes all four carry rows and totals across, in the one order the task keeps them in.

Bounds: everything here is an equality. The scalars are host arithmetic on a vector the task hands out, so they are compared as floats bit
for bit (nan equal to nan: the actuator group has a nan cost of transport where a mode barely moved); the checkpoint is compared as bytes.
What the vectors hold is held to the restatements by the per-statistic tests."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L

pytestmark = pytest.mark.gpu


def _same(got: dict, want: dict):
    assert got and set(got) == set(want)
    for k, x in want.items():
        assert got[k] == x or (x != x and got[k] != got[k]), (k, got[k], x)


def _state(task):
    """Per statistic, in the task's order: the carry rows and the totals, as bytes."""
    carriers = (task.episodes, task.tracking, task.gait, task.actuator)
    vectors = (task.episode_stats_vectors, task.tracking_stats_vectors, task.gait_stats_vectors, task.actuator_stats_vectors)
    return [(c.acc.cpu().numpy().tobytes(), v()[1].tobytes()) for c, v in zip(carriers, vectors)]


def test_the_four_statistics_together(tmp_path):
    """64 envs, 8-row rollouts, every env truncated after 5 steps: episodes end inside every rollout. tracking_settle_seconds = 2 rows, so
    that rows settle within such an episode and the tracking group is not empty."""
    from kbot_joystick_amd.host.actuator import actuator_scalars
    from kbot_joystick_amd.host.episode import episode_stats_scalars
    from kbot_joystick_amd.host.gait import gait_scalars
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
    from kbot_joystick_amd.host.tracking import tracking_scalars
    cfg = launch_config(num_envs=64, batch_size=64, hidden_size=64, num_passes=1, rollout_length_seconds=8 * 0.02, robot="kbot-headless", seed=5,
                        episode_stats=True, tracking_stats=True, tracking_settle_seconds=0.04, gait_stats=True, actuator_stats=True, record_state=True,
                        log_reward_components=True, termination_params={"episode_length": {"max_length_sec": 5 * 0.02}})
    a = HumanoidWalkingTask(cfg)
    assert (a.T, a.N) == (8, 64)
    dt = cfg.ctrl_dt
    for _ in range(2):
        a.train_iteration()
        sc = a.scalars()
        group = lambda prefix: {k: v for k, v in sc.items() if k.startswith(prefix)}
        ep_last, ep_total = a.episode_stats_vectors()
        assert ep_last[L.EPST["EPISODES"]] >= 64
        _same(group("episode/"), episode_stats_scalars(ep_last, dt, "episode/", terms=True))
        _same(group("episode_total/"), episode_stats_scalars(ep_total, dt, "episode_total/", terms=True))
        _same(group("track/"), tracking_scalars(a.tracking_stats_vectors()[0], "track/"))
        _same(group("gait/"), gait_scalars(a.gait_stats_vectors()[0], dt, "gait/"))
        _same(group("act/"), actuator_scalars(a.actuator_stats_vectors()[0], a.model_blob, dt, "act/", a.actuator.levels))
        assert "train/loss" in sc and any(k.startswith("reward/") for k in sc) and any(k.startswith("episode/reward/") for k in sc)
    # the scalar keys come in the order the task keeps the statistics in: episodes, tracking, gait, actuator
    first = {p: min(i for i, k in enumerate(sc) if k.startswith(p)) for p in ("episode/", "track/", "gait/", "act/")}
    assert first["episode/"] < first["track/"] < first["gait/"] < first["act/"]
    v = a.validate(num_envs=64, seconds=8 * 0.02)
    for prefix in ("valid/episode/", "valid/track/", "valid/gait/", "valid/act/"):
        assert any(k.startswith(prefix) for k in v), prefix
    assert "valid/reward_per_step" in v and any(k.startswith("valid/episode/reward/") for k in v)
    # checkpoint and resume: all four carry rows and totals, bit for bit, and again after one more iteration on both
    path = str(tmp_path / "ckpt.bin")
    a.save_checkpoint(path)
    b = HumanoidWalkingTask.load_task(path)
    assert all(np.frombuffer(acc, np.uint8).any() and np.frombuffer(total, np.uint8).any() for acc, total in _state(a)) and _state(a) == _state(b)
    a.train_iteration(); b.train_iteration()
    assert _state(a) == _state(b)
    a.close(); b.close()
