"""Gait statistics on the device (kbj_gait_stats; HumanoidWalkingTaskConfig.gait_stats): the per-env carry rows that live next to the env state,
the hand-over of one call's result to the host, the result vectors as logger scalars in seconds, metres and newtons - and the sweep, the gait
table: one line per scripted command, pooled from the per-env record of one call."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ..spec import constants, layout as L
from . import dist as dist_util
from .device_stats import DeviceStats
from .sweep import command_sweep, format_command_table

G, F, A, E = L.GAIT, L.GFOOT, L.GACC, L.GENV
FEET = ("left", "right")


def _moments(n: float, s: float, ss: float):
    """(mean, std) of n values with sum s and sum of squares ss, n > 0; the variance is clamped at 0 against the rounding of ss / n - mean^2."""
    mean = s / n
    return mean, math.sqrt(max(0.0, ss / n - mean * mean))


def gait_scalars(vec, ctrl_dt: float, prefix: str = "gait/") -> dict:
    """One KBJ_GAIT vector (kbj_model.h; layout.GAIT / GFOOT) as logger scalars. Per mode that has rows, `<prefix><mode>/...`:
    double_support_frac, single_support_frac, flight_frac; step_rate_hz (touchdowns of both feet per second of the mode's rows); repeat_frac
    (touchdowns of the foot that touched down last, per touchdown); torque_rms, torque_max; per foot `left_` / `right_`: swing_s_mean / _std
    / _max and stance_s_mean / _std / _max (seconds), duty (stance over stance + swing), clearance_m_mean / _max, force_n_mean (over the
    foot's contact rows) / _max; swing_asymmetry ((left - right) / (left + right) of the mean swing times). A scalar whose denominator is
    zero is omitted: a mean of nothing is not a number worth plotting."""
    vec = np.asarray(vec, np.float64)
    out = {}
    for m, mode in enumerate(constants.COMMAND_MODE_NAMES):
        b = vec[m * G["MODE_STRIDE"]:(m + 1) * G["MODE_STRIDE"]]
        rows = float(b[G["ROWS"]])
        if rows <= 0:
            continue
        p = f"{prefix}{mode}/"
        out[p + "double_support_frac"], out[p + "single_support_frac"], out[p + "flight_frac"] = (float(b[G[k]]) / rows for k in ("DOUBLE", "SINGLE", "FLIGHT"))
        feet = [b[G["FOOT"] + G["FOOT_STRIDE"] * f:G["FOOT"] + G["FOOT_STRIDE"] * (f + 1)] for f in range(2)]
        touchdowns = float(feet[0][F["TOUCHDOWNS"]] + feet[1][F["TOUCHDOWNS"]])
        out[p + "step_rate_hz"] = touchdowns / (rows * ctrl_dt)
        if touchdowns > 0:
            out[p + "repeat_frac"] = float(b[G["REPEATS"]]) / touchdowns
        out[p + "torque_rms"], out[p + "torque_max"] = math.sqrt(float(b[G["TORQUE_SQ"]]) / (rows * L.NU)), float(b[G["TORQUE_MAX"]])
        swing_mean = [None, None]
        for f, (side, x) in enumerate(zip(FEET, feet)):
            q = p + side + "_"
            for phase in ("SWING", "STANCE"):
                n = float(x[F[phase + "_N"]])
                if n > 0:
                    mean, std = _moments(n, float(x[F[phase + "_SUM"]]), float(x[F[phase + "_SUMSQ"]]))
                    name = phase.lower()
                    out[q + name + "_s_mean"], out[q + name + "_s_std"], out[q + name + "_s_max"] = mean * ctrl_dt, std * ctrl_dt, float(x[F[phase + "_MAX"]]) * ctrl_dt
                    if phase == "SWING":
                        swing_mean[f] = mean
                        out[q + "clearance_m_mean"], out[q + "clearance_m_max"] = float(x[F["CLEAR_SUM"]]) / n, float(x[F["CLEAR_MAX"]])
            both = float(x[F["STANCE_SUM"]] + x[F["SWING_SUM"]])
            if both > 0:
                out[q + "duty"] = float(x[F["STANCE_SUM"]]) / both
            contact = float(x[F["CONTACT_ROWS"]])
            if contact > 0:
                out[q + "force_n_mean"], out[q + "force_n_max"] = float(x[F["FORCE_SUM"]]) / contact, float(x[F["FORCE_MAX"]])
        if None not in swing_mean and swing_mean[0] + swing_mean[1] > 0:
            out[p + "swing_asymmetry"] = (swing_mean[0] - swing_mean[1]) / (swing_mean[0] + swing_mean[1])
    return out


class GaitStats(DeviceStats):
    """kbj_gait_stats over the rollouts of a run: the phase each foot of each env is in and since when (KBJ_GACC rows), the KBJ_GAIT vectors of
    the last rollout's rows and of all so far."""
    layout, acc_width, acc_key, total_key = dist_util.GAIT_STATS, A["SIZE"], "gait_acc", "gait_total"
    switch, prefix, total_prefix, valid_prefix = "gait_stats", "gait/", "gait_total/", "valid/gait/"

    def __init__(self, num_envs: int, ctrl_dt: float, device):
        self.ctrl_dt = ctrl_dt
        super().__init__(num_envs, device)

    @staticmethod
    def call(ctx, traj, acc, stats, env=None):
        ctx.gait_stats(traj, acc, stats, env)

    def scalars(self, vec, prefix: str) -> dict:
        return gait_scalars(vec, self.ctrl_dt, prefix)


# ---- the sweep ----
@dataclasses.dataclass
class GaitRecord:
    """What a gait sweep left on the device, for whoever wants more than the table: the aux rows [T + 1, N, AUX SIZE] and the per-env record
    [N, GENV SIZE] of kbj_gait_stats; env n follows command n % len(commands). `stats` is the call's KBJ_GAIT vector."""
    aux: torch.Tensor
    env: torch.Tensor
    stats: np.ndarray


def pool_gait_rows(rows, ctrl_dt: float) -> dict:
    """Gait figures of several envs together, from their KBJ_GENV rows [k, GENV SIZE]: counts and sums add up in float64, maxima are taken;
    nan where there is nothing to divide by."""
    r = np.asarray(rows, np.float64).reshape(-1, E["SIZE"])
    tot, top = r.sum(0), (r.max(0) if len(r) else np.zeros(E["SIZE"]))
    div = lambda a, b: float(a) / float(b) if b > 0 else float("nan")
    n = tot[G["ROWS"]]
    out, touchdowns = {}, 0.0
    for f, side in enumerate(FEET):
        x, hi = tot[E["FOOT"] + E["FOOT_STRIDE"] * f:], top[E["FOOT"] + E["FOOT_STRIDE"] * f:]
        out[side + "_swing_s"] = div(x[E["SWING_SUM"]], x[E["SWING_N"]]) * ctrl_dt
        out[side + "_stance_s"] = div(x[E["STANCE_SUM"]], x[E["STANCE_N"]]) * ctrl_dt
        out[side + "_clearance_m_mean"], out[side + "_clearance_m_max"] = div(x[E["CLEAR_SUM"]], x[E["SWING_N"]]), float(hi[E["CLEAR_MAX"]])
        out[side + "_force_n_max"] = float(hi[E["FORCE_MAX"]])
        touchdowns += x[E["TOUCHDOWNS"]]
    out["step_rate_hz"] = div(touchdowns, n * ctrl_dt)
    out["double_support_frac"], out["single_support_frac"], out["flight_frac"] = (div(tot[G[k]], n) for k in ("DOUBLE", "SINGLE", "FLIGHT"))
    out["repeat_frac"] = div(tot[G["REPEATS"]], touchdowns)
    out["torque_rms"] = math.sqrt(div(tot[G["TORQUE_SQ"]], n * L.NU))
    return out


def gait_sweep(task, commands=None, repeats: int = 2, seconds=None, seed_offset: int = 7919):
    """The sweep behind HumanoidWalkingTask.gait_sweep (see there): returns (entries, record) - one entry per command, and the GaitRecord of
    what the run left on the device. The rollout is tracking_sweep's (host/sweep.py sweep_rollout under a ScriptedCommand term); one
    kbj_gait_stats call on a fresh carry then gives every env's totals."""
    dev, dt = task.device, task.config.ctrl_dt
    with command_sweep(task, "gait_sweep", commands, repeats, seconds, seed_offset) as (ctx, tr, n, T, entries):
        env = torch.empty(n, E["SIZE"], device=dev)
        stats = GaitStats.fresh(ctx, tr.c, n, dev, env=env)
        ctx.synchronize()
        rows, vec = env.cpu().numpy(), stats.cpu().numpy()
    return entries(lambda envs: pool_gait_rows(rows[envs], dt)), GaitRecord(tr.aux, env, vec)


GAIT_TABLE_COLUMNS = (("L swing s", "left_swing_s"), ("R swing s", "right_swing_s"), ("L stance s", "left_stance_s"), ("R stance s", "right_stance_s"),
                      ("L clear m", "left_clearance_m_mean"), ("R clear m", "right_clearance_m_mean"), ("L clr max", "left_clearance_m_max"),
                      ("R clr max", "right_clearance_m_max"), ("L peak N", "left_force_n_max"), ("R peak N", "right_force_n_max"), ("steps/s", "step_rate_hz"),
                      ("double", "double_support_frac"), ("single", "single_support_frac"), ("flight", "flight_frac"), ("repeat", "repeat_frac"),
                      ("torque rms", "torque_rms"), ("fail/s", "failures_per_s"))


def format_gait_table(entries) -> str:
    """gait_sweep's result as a text table: one line per command (its non-zero components by name), then per foot the mean swing and stance
    time, mean and largest clearance and peak force, the step rate, the three support shares, the repeat share, the torque level and the
    failures per second ("-" where there was nothing to average)."""
    return format_command_table(entries, GAIT_TABLE_COLUMNS)
