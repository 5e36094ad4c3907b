"""Scripted disturbances: user-written Event terms, and the push-recovery sweep built on one.

    python examples/push_events.py [iterations]

  Event   `initial_event_state(state, curriculum_level, rng)` (optional),
          `__call__(state, event_state, curriculum_level, rng) -> (push, event_state)`      -> extra_events

The reference lists its events in get_events (train.py:1134-1144: one ForcePushEvent), but ksim's Event class is not in its tree, so this
protocol is this build's own (host/user_terms.py apply_events). `push` is None or a `PushRequest(mask [N] bool, wrench [N, 6], steps [N])`:
force then torque in the world frame, applied at the base for the next `steps` control steps (kbj_env_set_push). The built-in event keeps
drawing its own pushes beside a user term unless the term also hands `next=PUSH_NEVER` to the envs it masks - and does so again after
every in-episode reset, which re-arms the built-in schedule (host/push.ScriptedPush, the term behind `task.push_sweep()`, does).
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kbot_joystick_amd.host.push import ScriptedPush, format_push_table      # noqa: F401 (ScriptedPush: the sweep's own term, shown here by name)
from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
from kbot_joystick_amd.host.traj_view import PushRequest


class PeriodicShove:
    """Every `period` seconds of an env's episode a horizontal shove of `force` newtons for `duration` seconds, its heading drawn afresh per
    env and shove. The event state is the env's count of control steps since its last shove (it starts again with the episode)."""

    def __init__(self, period: float = 2.0, force: float = 120.0, duration: float = 0.1, ctrl_dt: float = 0.02):
        self.every, self.force, self.steps = max(1, round(period / ctrl_dt)), force, max(1, round(duration / ctrl_dt))

    def initial_event_state(self, state, curriculum_level, rng):
        return torch.zeros(state.N, device=state.done.device)

    def __call__(self, state, since, curriculum_level, rng):
        dev = state.done.device
        since = since + 1
        due = since >= self.every
        heading = torch.rand(state.N, device=dev, generator=rng) * (2 * math.pi)
        wrench = torch.zeros(state.N, 6, device=dev)
        wrench[:, 0], wrench[:, 1] = self.force * torch.cos(heading), self.force * torch.sin(heading)
        return PushRequest(due, wrench, torch.full((state.N,), float(self.steps), device=dev)), torch.where(due, torch.zeros_like(since), since)


def main(iterations: int = 2, num_envs: int = 256):
    cfg = launch_config(num_envs=num_envs, batch_size=min(64, num_envs), hidden_size=64, rollout_length_seconds=2.0, robot="kbot-headless")
    shove = PeriodicShove(period=0.5, ctrl_dt=cfg.ctrl_dt)
    task = HumanoidWalkingTask(cfg, extra_events={"periodic_shove": shove})
    print("events:", ", ".join(task.get_events()))
    for it in range(iterations):
        task.train_iteration()
        sc = task.scalars()
        print(f"iter {it + 1}: reward/step {sc['train/reward_per_step']:.4f}  failures/step {sc['train/failures_per_step']:.4f}  loss {sc['train/loss']:.4f}", flush=True)
    assert torch.isfinite(task.params).all()
    # the robustness table of the policy as it stands (two iterations old: expect VOID and FELL): a small grid, short times
    entries, record = task.push_sweep(forces=(0.0, 100.0, 200.0), directions_deg=(0, 90, 180, 270), duration=0.2, push_at=0.5, window=1.0, hold=0.2, repeats=4)
    print(format_push_table(entries))
    assert sum(e["valid"] + e["void"] for e in entries) == record.rec.shape[0]
    task.close()
    print("push events ok")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2)
