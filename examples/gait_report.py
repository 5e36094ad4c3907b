"""How the robot walks, as numbers: the gait statistics of a training run and the gait table of its policy.

    python examples/gait_report.py [iterations]

`gait_stats=True` makes every rollout end with one kbj_gait_stats call; its result arrives in `scalars()` as `gait/<mode>/...` - swing and
stance times in seconds, duty factor, step rate, support shares, clearance in metres, ground force in newtons, torque level - per command
mode. `task.gait_sweep()` runs a scripted command per env on a context of its own and pools one line per command (it needs no switch).
A policy a few iterations old does not walk: expect long stances, few steps and `-` where nothing was counted.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kbot_joystick_amd.host.gait import format_gait_table
from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config


def main(iterations: int = 2, num_envs: int = 256):
    cfg = launch_config(num_envs=num_envs, batch_size=min(64, num_envs), hidden_size=64, rollout_length_seconds=2.0, robot="kbot-headless", gait_stats=True)
    task = HumanoidWalkingTask(cfg)
    for it in range(iterations):
        task.train_iteration()
        sc = task.scalars()
        print(f"iter {it + 1}: reward/step {sc['train/reward_per_step']:.4f}  loss {sc['train/loss']:.4f}", flush=True)
    assert torch.isfinite(task.params).all()
    forward = {k: v for k, v in sc.items() if k.startswith("gait/forward/")}
    for k in sorted(forward):
        print(f"  {k} = {forward[k]:.4f}")
    assert any(k.startswith("gait/") for k in sc)
    entries = task.gait_sweep(seconds=3.0)          # the default command grid, two envs per command
    print(format_gait_table(entries))
    assert len(entries) == 15
    task.close()
    print("gait report ok")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2)
