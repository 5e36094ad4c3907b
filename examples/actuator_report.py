"""What a policy asks of the motors, as numbers: the actuator statistics of a training run, per joint, and the actuator table of its policy.

    python examples/actuator_report.py [checkpoint | iterations]

With a checkpoint path the task is loaded from it (kbj_actuator_stats then runs in the sweep only, unless the run was saved with the switch
on); otherwise a small task is created and trained for a few iterations. `actuator_stats=True` (with `record_state=True`: joint positions
and speeds come from the state record) makes every rollout end with one kbj_actuator_stats call; its result arrives in `scalars()` as
`act/<mode>/...` - mean |P| and positive power in watts, cost of transport, torque rms, the share of rows with a joint at its torque level
or at a stop, the action rate, the joint nearest its level - per command mode, and `task.actuator_stats(per_joint=True)` gives one line per
joint. `task.actuator_sweep()` runs a scripted command per env on a context of its own and pools one line per command (it needs no switch).
The levels (0.9 of the torque limit, no speed limit, 2 degrees inside a joint's range) are settings of this build.
A policy a few iterations old flails: expect torques at the level on most rows.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kbot_joystick_amd.host.actuator import format_actuator_joint_table, format_actuator_table
from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config


def main(arg: str = "2", num_envs: int = 256):
    if os.path.exists(arg):
        task = HumanoidWalkingTask.load_task(arg)
        print(f"loaded {arg}: iteration {task.iteration}")
    else:
        cfg = launch_config(num_envs=num_envs, batch_size=min(64, num_envs), hidden_size=64, rollout_length_seconds=2.0, robot="kbot-headless",
                            actuator_stats=True, record_state=True)
        task = HumanoidWalkingTask(cfg)
        for it in range(int(arg)):
            task.train_iteration()
            sc = task.scalars()
            print(f"iter {it + 1}: reward/step {sc['train/reward_per_step']:.4f}  loss {sc['train/loss']:.4f}", flush=True)
        assert torch.isfinite(task.params).all() and any(k.startswith("act/") for k in sc)
        for k in sorted(k for k in sc if k.startswith("act/forward/")):
            print(f"  {k} = {sc[k]:.4f}")
    if task.actuator is not None and task.iteration > 0:
        print(format_actuator_joint_table(task.actuator_stats(total=True, per_joint=True)))      # all rollouts since creation or resume
    entries = task.actuator_sweep(seconds=3.0)          # the default command grid, two envs per command
    print(format_actuator_table(entries))
    assert len(entries) == 15
    task.close()
    print("actuator report ok")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "2")
