"""Episode accounting on the device (kbj_episode_stats; HumanoidWalkingTaskConfig.episode_stats): the per-env accumulator rows that live next
to the env state, the hand-over of one call's result to the host, and the result vectors as logger scalars."""
from __future__ import annotations

import math

import numpy as np
import torch

from ..spec import constants, layout as L
from . import dist as dist_util


def episode_stats_scalars(vec, ctrl_dt: float, prefix: str = "episode/", terms: bool = False) -> dict:
    """One KBJ_EPST vector (kbj_model.h; layout.EPST) as logger scalars. Means over the finished episodes are omitted when there are none
    (and the time to failure when none of them failed): a mean of nothing is not a number worth plotting."""
    E = L.EPST
    n = float(vec[E["EPISODES"]])
    out = {prefix + "count": n}
    if n <= 0:
        return out
    mean = float(vec[E["RETURN_SUM"]]) / n
    out[prefix + "return_mean"] = mean
    out[prefix + "return_std"] = math.sqrt(max(float(vec[E["RETURN_SUMSQ"]]) / n - mean * mean, 0.0))
    out[prefix + "return_min"], out[prefix + "return_max"] = float(vec[E["RETURN_MIN"]]), float(vec[E["RETURN_MAX"]])
    out[prefix + "length_s_mean"] = float(vec[E["LENGTH_SUM"]]) / n * ctrl_dt
    out[prefix + "length_s_max"] = float(vec[E["LENGTH_MAX"]]) * ctrl_dt
    fails = float(vec[E["FAIL_HEIGHT"]] + vec[E["FAIL_OTHER"]])
    if fails > 0:
        out[prefix + "time_to_failure_s_mean"] = float(vec[E["FAIL_LENGTH_SUM"]]) / fails * ctrl_dt
    for key, slot in (("frac_fail_height", "FAIL_HEIGHT"), ("frac_fail_other", "FAIL_OTHER"), ("frac_truncated", "TRUNCATED")):
        out[prefix + key] = float(vec[E[slot]]) / n
    if terms:
        for k, name in enumerate(constants.REWARD_NAMES):
            out[f"{prefix}reward/{name}"] = float(vec[E["TERM_SUM"] + k]) / n
    return out


def fresh_episode_stats(ctx, traj, num_envs: int, device) -> torch.Tensor:
    """kbj_episode_stats on a trajectory whose episodes all start with it (every validation rollout): its KBJ_EPST vector, on the device."""
    acc = torch.zeros(num_envs, L.EACC["SIZE"], device=device)
    stats = torch.zeros(L.EPST["SIZE"], dtype=torch.float64, device=device)
    ctx.episode_stats(traj, acc, stats)
    return stats


class EpisodeStats:
    """Per-env accumulator rows (`acc`, carried across rollouts and through checkpoints), one call's result (`stats`), and on the host the
    last rollout's vector and the totals since creation / resume. The result comes back through a pinned buffer behind the kernel (no sync
    in the loop); it is folded into the totals when the next rollout starts or when somebody asks."""

    def __init__(self, num_envs: int, device):
        self.acc = torch.zeros(num_envs, L.EACC["SIZE"], device=device)
        self.stats = torch.zeros(L.EPST["SIZE"], dtype=torch.float64, device=device)
        self._host = torch.zeros(L.EPST["SIZE"], dtype=torch.float64).pin_memory()
        self._event = torch.cuda.Event()
        self._pending = False
        self._last = dist_util.empty_episode_stats()
        self._total = dist_util.empty_episode_stats()

    def after_rollout(self, ctx, traj):
        """Account the rollout in `traj` (behind the user rewards, so that they count; user terminations are in the DONE column already)."""
        self._fold()
        ctx.episode_stats(traj, self.acc, self.stats)
        self._host.copy_(self.stats, non_blocking=True)
        self._event.record()
        self._pending = True

    def _fold(self):
        """The last kbj_episode_stats result, once its copy has landed, becomes `_last` and joins the totals."""
        if self._pending:
            self._event.synchronize()
            self._last = self._host.numpy().copy()
            self._total = dist_util.combine_episode_stats([self._total, self._last])
            self._pending = False

    def vectors(self):
        """(last, total): the KBJ_EPST vectors (float64 numpy) of the episodes that finished in the last rollout and of all so far."""
        self._fold()
        return self._last, self._total

    def checkpoint_state(self) -> dict:
        """Episodes in flight and the totals so far (the last rollout's own vector is not state)."""
        self._fold()
        return dict(ep_acc=self.acc.cpu().numpy(), ep_total=self._total.copy())

    def load_checkpoint_state(self, x):
        """The members when the saved run kept them (same env count), else from zero - episodes already running are then counted from here
        on (an old checkpoint, a run saved with the switch off, a model-only file)."""
        self._pending = False
        self._last = dist_util.empty_episode_stats()
        if "ep_acc" in x and "ep_total" in x and tuple(x["ep_acc"].shape) == tuple(self.acc.shape) and x["ep_total"].shape == (L.EPST["SIZE"],):
            self.acc.copy_(torch.from_numpy(np.ascontiguousarray(x["ep_acc"], np.float32)))
            self._total = np.array(x["ep_total"], np.float64)
        else:
            self.acc.zero_()
            self._total = dist_util.empty_episode_stats()
