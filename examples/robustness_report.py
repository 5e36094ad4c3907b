"""What a policy does on a robot that is not the model, as numbers: the robustness table of a policy.

    python examples/robustness_report.py [checkpoint | iterations]

With a checkpoint path the task is loaded from it; otherwise a small task is created and trained for a few iterations.
`task.robustness_sweep()` runs one case per (perturbation, command) on a context of its own: half and a quarter of the floor friction, the
mass 15 % off, 5 kg on the torso, softer and stiffer gains, motors at 70 % and 50 % torque, no and a full step of action latency, twice the
armature, three times the joint friction, a weak left leg - each standing, walking forward at half and full range and turning. Every env's
model row is written by kbj_env_perturb and written again after every in-episode reset; kbj_robustness then gives per case the share of envs
that never fell, the falls per second, the time of the first fall and the settled-row tracking errors. Cases marked `*` lie outside what the
training randomisers draw. The perturbations are settings of this build, not measured thresholds, and the table has not been taken on a
trained policy: a policy a few iterations old falls in every case.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kbot_joystick_amd.host.robustness import Perturbation, format_robustness_table
from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config


def main(arg: str = "2", num_envs: int = 256):
    if os.path.exists(arg):
        task = HumanoidWalkingTask.load_task(arg)
        print(f"loaded {arg}: iteration {task.iteration}")
    else:
        cfg = launch_config(num_envs=num_envs, batch_size=min(64, num_envs), hidden_size=64, rollout_length_seconds=2.0, robot="kbot-headless")
        task = HumanoidWalkingTask(cfg)
        for it in range(int(arg)):
            task.train_iteration()
            sc = task.scalars()
            print(f"iter {it + 1}: reward/step {sc['train/reward_per_step']:.4f}  loss {sc['train/loss']:.4f}", flush=True)
        assert torch.isfinite(task.params).all()
    entries, record = task.robustness_sweep(repeats=2, seconds=3.0)          # the default perturbations and commands, two envs per case
    print(format_robustness_table(entries))
    assert len(entries) == 16 * 4 and all(x["envs"] == 2 for x in entries)
    # a case of one's own: a heavy backpack carried high and behind, on tired arms
    own = Perturbation("backpack", payload_kg=6.0, com_shift=(-0.05, 0.0, 0.08), torque_scale={"left_arm": 0.7, "right_arm": 0.7})
    entries, _ = task.robustness_sweep(perturbations=[Perturbation("nominal"), own], commands=[(), (0.5,)], repeats=4, seconds=3.0)
    print(format_robustness_table(entries))
    task.close()
    print("robustness report ok")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "2")
