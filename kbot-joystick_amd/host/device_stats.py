"""The host carrier of a statistic the device accumulates over rollouts (kbj_episode_stats, kbj_tracking_stats, kbj_gait_stats, kbj_actuator_stats;
host/episode.py, host/tracking.py, host/gait.py and host/actuator.py declare one each): the per-env rows that live next to the env state, the hand-over of
one call's result to the host, the totals - and the same call on rows of its own, for a trajectory that stands alone."""
from __future__ import annotations

import numpy as np
import torch


def fresh_stats(layout, acc_width: int, call, num_envs: int, device) -> torch.Tensor:
    """`call(acc, stats)` on zeroed per-env rows [num_envs, acc_width] - a trajectory whose episodes all start with it (every validation
    and sweep rollout): its vector of `layout` (dist.StatsLayout), on the device."""
    acc = torch.zeros(num_envs, acc_width, device=device)
    stats = torch.zeros(layout.empty().size, dtype=torch.float64, device=device)
    call(acc, stats)
    return stats


class DeviceStats:
    """Per-env rows (`acc` [num_envs, acc_width], carried across rollouts and through checkpoints), one call's result (`stats`, a vector of
    `layout`: dist.StatsLayout), and on the host the last rollout's vector and the totals since creation / resume. The result comes back
    through a pinned buffer behind the kernel (no sync in the loop); it is folded into the totals when the next rollout starts or when
    somebody asks. Checkpoints hold `acc` and the totals under `acc_key` and `total_key`.

    A subclass is the whole declaration of a statistic (HumanoidWalkingTask reads nothing else): as class attributes `layout`, `acc_width`,
    `acc_key`, `total_key`, the config field `switch` that turns it on, and the key prefixes `prefix` (the last rollout), `total_prefix`
    and `valid_prefix` (validate()); `call(ctx, traj, acc, stats, *settings, **outputs)`, a static method, the ONE place that spells the ABI
    call (`outputs`: the optional per-row or per-env record a sweep asks for); `scalars(vec, prefix)`, a vector as logger scalars with the
    carrier's own settings bound. `settings`: what the constructor was given for `call` (the settle rows, the levels)."""
    settings = ()

    def __init__(self, num_envs: int, device):
        size = self.layout.empty().size
        self.acc = torch.zeros(num_envs, self.acc_width, device=device)
        self.stats = torch.zeros(size, dtype=torch.float64, device=device)
        self._host = torch.zeros(size, dtype=torch.float64).pin_memory()
        self._event = torch.cuda.Event()
        self._pending = False
        self._last = self.layout.empty()
        self._total = self.layout.empty()

    @classmethod
    def fresh(cls, ctx, traj, num_envs: int, device, *settings, **outputs) -> torch.Tensor:
        """The call on a trajectory whose episodes all start with it (every validation and sweep rollout; no carrier needed): its vector,
        on the device."""
        return fresh_stats(cls.layout, cls.acc_width, lambda acc, stats: cls.call(ctx, traj, acc, stats, *settings, **outputs), num_envs, device)

    def valid_scalars(self, vec) -> dict:
        """validate()'s scalars of such a vector."""
        return self.scalars(vec, self.valid_prefix)

    def after_rollout(self, ctx, traj):
        """Account the rollout in `traj` (behind the user rewards and terminations, so that they count)."""
        self._fold()
        self.call(ctx, traj, self.acc, self.stats, *self.settings)
        self._host.copy_(self.stats, non_blocking=True)
        self._event.record()
        self._pending = True

    def _fold(self):
        """The last call's result, once its copy has landed, becomes `_last` and joins the totals."""
        if self._pending:
            self._event.synchronize()
            self._last = self._host.numpy().copy()
            self._total = self.layout.combine([self._total, self._last])
            self._pending = False

    def vectors(self):
        """(last, total): the vectors (float64 numpy) of the last rollout and of all rollouts so far."""
        self._fold()
        return self._last, self._total

    def checkpoint_state(self) -> dict:
        """What is in flight per env and the totals so far (the last rollout's own vector is not state)."""
        self._fold()
        return {self.acc_key: self.acc.cpu().numpy(), self.total_key: self._total.copy()}

    def load_checkpoint_state(self, x):
        """The members when the saved run kept them (same env count), else from zero - what is in flight is then counted from here on (an old
        checkpoint, a run saved with the switch off, a model-only file)."""
        a, t = self.acc_key, self.total_key
        self._pending = False
        self._last = self.layout.empty()
        if a in x and t in x and tuple(x[a].shape) == tuple(self.acc.shape) and x[t].shape == self._last.shape:
            self.acc.copy_(torch.from_numpy(np.ascontiguousarray(x[a], np.float32)))
            self._total = np.array(x[t], np.float64)
        else:
            self.acc.zero_()
            self._total = self.layout.empty()
