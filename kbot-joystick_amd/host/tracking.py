"""Command-tracking errors on the device (kbj_tracking_stats; HumanoidWalkingTaskConfig.tracking_stats): the per-env carry rows that live next
to the env state, the hand-over of one call's result to the host, the result vectors as logger scalars - and the sweep, the joystick
response table (its scripted Command term and default command grid are host/sweep.py's, shared with the gait and actuator sweeps)."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ..spec import constants, layout as L
from . import dist as dist_util
from .device_stats import DeviceStats
from .sweep import command_label, command_mode, command_sweep, default_command_grid      # noqa: F401 (command_mode, default_command_grid: re-exported)

K, A, R = L.TRK, L.TACC, L.TERR


def settle_steps(settle_seconds: float, ctrl_dt: float) -> int:
    """Rows a command must have been held for before a row counts (kbj_tracking_stats settle_steps)."""
    return max(0, int(round(settle_seconds / ctrl_dt)))


def tracking_scalars(vec, prefix: str = "track/") -> dict:
    """One KBJ_TRK vector (kbj_model.h; layout.TRK) as logger scalars: per mode that has settled rows the mean, rms and maximum of every error
    over them, the mode's share of all rows and the settled share of its rows. A mode without settled rows is omitted: a mean of nothing
    is not a number worth plotting."""
    vec = np.asarray(vec, np.float64)
    rows_all = sum(float(vec[m * K["MODE_STRIDE"] + K["ROWS"]]) for m in range(L.CMODE["COUNT"]))
    out = {}
    for m, mode in enumerate(constants.COMMAND_MODE_NAMES):
        b = vec[m * K["MODE_STRIDE"]:(m + 1) * K["MODE_STRIDE"]]
        rows, n = float(b[K["ROWS"]]), float(b[K["SETTLED"]])
        if n <= 0:
            continue
        for k, name in enumerate(constants.TRACKING_ERROR_NAMES):
            out[f"{prefix}{mode}/{name}_mean"] = float(b[K["SUM"] + k]) / n
            out[f"{prefix}{mode}/{name}_rms"] = math.sqrt(float(b[K["SUMSQ"] + k]) / n)
            out[f"{prefix}{mode}/{name}_max"] = float(b[K["MAX"] + k])
        out[f"{prefix}{mode}/rows_frac"] = rows / rows_all
        out[f"{prefix}{mode}/settled_frac"] = n / rows
    return out


class TrackingStats(DeviceStats):
    """kbj_tracking_stats over the rollouts of a run: the command each env holds and for how long (KBJ_TACC rows), the KBJ_TRK vectors of the
    last rollout's rows and of all so far. A row counts once its command has been held for `settle_steps` rows."""
    layout, acc_width, acc_key, total_key = dist_util.TRACKING_STATS, A["SIZE"], "trk_acc", "trk_total"
    switch, prefix, total_prefix, valid_prefix = "tracking_stats", "track/", "track_total/", "valid/track/"

    def __init__(self, num_envs: int, steps: int, device):
        self.settle_steps, self.settings = steps, (steps,)
        super().__init__(num_envs, device)

    @staticmethod
    def call(ctx, traj, acc, stats, steps: int, err=None):
        ctx.tracking_stats(traj, steps, acc, stats, err)

    def scalars(self, vec, prefix: str) -> dict:
        return tracking_scalars(vec, prefix)


# ---- the sweep ----
@dataclasses.dataclass
class SweepRecord:
    """What a sweep left on the device, for whoever wants more than the table: the aux rows [T + 1, N, AUX SIZE] and the per-row output
    [T, N, TERR SIZE] of kbj_tracking_stats; env n follows command n % len(commands)."""
    aux: torch.Tensor
    err: torch.Tensor
    stats: np.ndarray


def tracking_sweep(task, commands=None, repeats: int = 2, seconds=None, settle_seconds=None, seed_offset: int = 7919):
    """The sweep behind HumanoidWalkingTask.tracking_sweep (see there): returns (entries, record) - one entry per command, and the SweepRecord
    of what the run left on the device. Every call builds a context of its own for its env count and length and closes it again
    (host/sweep.py sweep_rollout)."""
    cfg, dev = task.config, task.device
    steps = settle_steps(cfg.tracking_settle_seconds if settle_seconds is None else settle_seconds, cfg.ctrl_dt)
    with command_sweep(task, "tracking_sweep", commands, repeats, seconds, seed_offset) as (ctx, tr, n, T, entries):
        err = torch.empty(T, n, R["SIZE"], device=dev)
        stats = TrackingStats.fresh(ctx, tr.c, n, dev, steps, err=err)
        ctx.synchronize()
        e, vec = err.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    settled = e[:, :, R["SETTLED"]] != 0

    def settled_means(envs):      # per env the mean over its settled rows, then the mean over the repeats that have any
        out = {}
        for k, name in enumerate(constants.TRACKING_ERROR_NAMES):
            means = [e[settled[:, j], j, k].mean() for j in envs if settled[:, j].any()]
            out[name] = float(np.mean(means)) if means else float("nan")
        out["settled_rows"] = int(sum(settled[:, j].sum() for j in envs))
        return out
    return entries(settled_means), SweepRecord(tr.aux, err, vec)


def format_tracking_table(entries) -> str:
    """tracking_sweep's result as a text table: one line per command (its non-zero components by name), the five settled-row mean errors,
    the settled row count and the failures per second."""
    names = constants.TRACKING_ERROR_NAMES
    labels = [command_label(x["command"]) for x in entries]
    w = max([len("command")] + [len(s) for s in labels])
    lines = [f"{'command':{w}s}  {'mode':10s}" + "".join(f"  {n:>12s}" for n in names) + f"  {'settled':>8s}  {'fail/s':>8s}"]
    for s, x in zip(labels, entries):
        lines.append(f"{s:{w}s}  {x['mode']:10s}" + "".join(f"  {x[n]:12.4f}" for n in names) + f"  {x['settled_rows']:8d}  {x['failures_per_s']:8.3f}")
    return "\n".join(lines)
