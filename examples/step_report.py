"""What the robot does when the stick moves, as numbers: the step-response table of a policy.

    python examples/step_report.py [iterations]

`task.step_sweep()` runs one scheduled command change per env on a context of its own - starts, stops, a speed-up, the reversal and a turn
reversal at the config's full command ranges, four envs per transition - and ONE kbj_step_response call scores them on the device: rise
time, overshoot, settling time, the travel until settled (the stopping distance of a stop), the cross-coupling into the channels that did
not move, and the falls. The bands and levels are settings, echoed above the table, not measured thresholds. A policy a few iterations old
does not follow its stick: expect `void` (it was not on its old command when the stick moved), falls, and `-` where nothing was counted.
The record beside the entries holds the signal and every env's figures for whoever wants more than the table.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kbot_joystick_amd.host.step import format_step_table
from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
from kbot_joystick_amd.spec import constants, layout as L


def main(iterations: int = 2, num_envs: int = 256):
    cfg = launch_config(num_envs=num_envs, batch_size=min(64, num_envs), hidden_size=64, rollout_length_seconds=2.0, robot="kbot-headless")
    task = HumanoidWalkingTask(cfg)
    for it in range(iterations):
        task.train_iteration()
        sc = task.scalars()
        print(f"iter {it + 1}: reward/step {sc['train/reward_per_step']:.4f}  loss {sc['train/loss']:.4f}", flush=True)
    assert torch.isfinite(task.params).all()
    entries, record = task.step_sweep(step_at=2.0, window=3.0)          # the default transitions, four envs each
    print(format_step_table(entries))
    assert len(entries) == 10 and all(e["valid"] + e["void"] == 4 for e in entries)
    outcomes = record.rec[:, L.SREC["OUTCOME"]].cpu().numpy().astype(int)
    print("outcomes:", {name: int((outcomes == k).sum()) for k, name in enumerate(constants.STEP_OUTCOME_NAMES)})
    task.close()
    print("step report ok")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2)
