"""Episode accounting on the device (kbj_episode_stats; HumanoidWalkingTaskConfig.episode_stats): the per-env accumulator rows that live next
to the env state, the hand-over of one call's result to the host, and the result vectors as logger scalars."""
from __future__ import annotations

import math

from ..spec import constants, layout as L
from . import dist as dist_util
from .device_stats import DeviceStats


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


class EpisodeStats(DeviceStats):
    """kbj_episode_stats over the rollouts of a run: the episodes in flight per env (KBJ_EACC rows), the KBJ_EPST vectors of the episodes that
    finished in the last rollout and of all so far. `terms`: the trajectory keeps the reward terms (log_reward_components), so the vectors
    hold their episodic sums."""
    layout, acc_width, acc_key, total_key = dist_util.EPISODE_STATS, L.EACC["SIZE"], "ep_acc", "ep_total"
    switch, prefix, total_prefix, valid_prefix = "episode_stats", "episode/", "episode_total/", "valid/episode/"

    def __init__(self, num_envs: int, ctrl_dt: float, terms: bool, device):
        self.ctrl_dt, self.terms = ctrl_dt, terms
        super().__init__(num_envs, device)

    @staticmethod
    def call(ctx, traj, acc, stats):
        ctx.episode_stats(traj, acc, stats)

    def scalars(self, vec, prefix: str, terms=None) -> dict:
        return episode_stats_scalars(vec, self.ctrl_dt, prefix, self.terms if terms is None else terms)

    def valid_scalars(self, vec) -> dict:
        return self.scalars(vec, self.valid_prefix, terms=True)      # validate()'s trajectory always keeps the reward terms
