"""How the robot follows a stick that keeps moving, as numbers: the frequency-response table of a policy.

    python examples/frequency_report.py [iterations]

`task.frequency_sweep()` moves one command word of every env sinusoidally on a context of its own - each of the three channels around
standing at half its range and forward around half speed at a quarter, at six periods from 0.25 to 6.25 Hz, four envs per case - and ONE
kbj_frequency_response call sums every response channel against the recorded command and against the same command a quarter period
earlier. The host forms gain, lag, delay, coherence and the cross-coupling from those sums, and the -3 dB bandwidth per operating point.
`min_amp` and the grid are settings, echoed above the table, not measured thresholds; the figures are linear-systems language applied to a
nonlinear walker, and the coherence says how far to trust them. A policy a few iterations old does not follow its stick: expect falls,
a gain near zero, a coherence near zero and `-` where nothing was measured. The record beside the entries holds the signal and every env's
sums for whoever wants more than the table.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kbot_joystick_amd.host.frequency import DEFAULT_PERIODS, format_frequency_table
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
    entries, record = task.frequency_sweep(start_at=1.0, settle=1.0)      # the default operating points and periods, four envs each
    print(format_frequency_table(entries))
    assert len(entries) == 4 * len(DEFAULT_PERIODS) and all(e["valid"] + e["void"] == 4 for e in entries)
    outcomes = record.rec[:, L.FREC["OUTCOME"]].cpu().numpy().astype(int)
    print("outcomes:", {name: int((outcomes == k).sum()) for k, name in enumerate(constants.FREQUENCY_OUTCOME_NAMES)})
    task.close()
    print("frequency report ok")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2)
