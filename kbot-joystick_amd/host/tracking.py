"""Command-tracking errors on the device (kbj_tracking_stats; HumanoidWalkingTaskConfig.tracking_stats): the per-env carry rows that live next
to the env state, the hand-over of one call's result to the host, the result vectors as logger scalars - and the sweep, the joystick
response table: a scripted Command term that holds one command per env through in-episode resets, the default command grid, the table."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ..spec import constants, layout as L
from . import dist as dist_util
from .device_stats import DeviceStats, fresh_stats
from .sweep import command_label, command_table, failures_per_s, held_command_rollout

K, A, R = L.TRK, L.TACC, L.TERR


def settle_steps(settle_seconds: float, ctrl_dt: float) -> int:
    """Rows a command must have been held for before a row counts (kbj_tracking_stats settle_steps)."""
    return max(0, int(round(settle_seconds / ctrl_dt)))


def command_mode(cmd) -> int:
    """The KBJ_CMODE of one command (include/kbj.h kbj_tracking_stats): which of cmd[0:3] are non-zero, and whether any of cmd[3:16] is."""
    c = np.asarray(cmd, np.float32)
    nz, pose = c[:3] != 0, bool((c[3:] != 0).any())
    if not nz.any():
        return L.CMODE["STAND_BEND"] if pose else L.CMODE["STAND"]
    if pose or nz.sum() != 1:
        return L.CMODE["OMNI"]
    return int(np.argmax(nz))


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


def fresh_tracking_stats(ctx, traj, num_envs: int, steps: int, device, err=None) -> torch.Tensor:
    """kbj_tracking_stats on a trajectory whose episodes all start with it (every validation rollout): its KBJ_TRK vector, on the device."""
    return fresh_stats(dist_util.TRACKING_STATS, A["SIZE"], lambda acc, stats: ctx.tracking_stats(traj, steps, acc, stats, err), num_envs, device)


class TrackingStats(DeviceStats):
    """kbj_tracking_stats over the rollouts of a run: the command each env holds and for how long (KBJ_TACC rows), the KBJ_TRK vectors of the
    last rollout's rows and of all so far. A row counts once its command has been held for `settle_steps` rows."""

    def __init__(self, num_envs: int, steps: int, device):
        self.settle_steps = steps
        super().__init__(num_envs, A["SIZE"], dist_util.TRACKING_STATS, lambda ctx, traj, acc, stats: ctx.tracking_stats(traj, self.settle_steps, acc, stats),
                         "trk_acc", "trk_total", device)


# ---- the sweep ----
class ScriptedCommand:
    """A Command term (train.py:724, 768) that holds one fixed command per env: `initial_command` is the env's row of `table` [N, 16],
    `__call__` the previous command - so a command survives an in-episode reset, after which the kernel's own reset (command_mode = 1)
    has returned the env to the context's single fixed_command."""

    def __init__(self, table: torch.Tensor):
        self.table = table

    def initial_command(self, state, curriculum_level, rng):
        return self.table

    def __call__(self, prev_command, state, curriculum_level, rng):
        return prev_command


def default_command_grid(kcfg) -> list:
    """The sweep's default commands, from the command ranges of a kbj_config (train.py:1211-1217): stand; forward (vx_hi), backward (vx_lo),
    left (vy_hi), right (vy_lo), turn left (wz_hi) and turn right (wz_lo), each at half and at full range; one omni command (half of vx_hi,
    vy_hi and wz_hi at once); one stand-bend command (half of bh_lo, rx_hi and ry_hi). 15 rows of 16 floats, arms at zero."""
    def cmd(**kw):
        c = [0.0] * L.NCMD
        for k, v in kw.items():
            c[constants.COMMAND_NAMES.index(k)] = float(v)
        return tuple(c)
    grid = [cmd()]
    for name, end in (("xvel", kcfg.vx_hi), ("xvel", kcfg.vx_lo), ("yvel", kcfg.vy_hi), ("yvel", kcfg.vy_lo), ("yawrate", kcfg.wz_hi), ("yawrate", kcfg.wz_lo)):
        grid += [cmd(**{name: 0.5 * end}), cmd(**{name: end})]
    grid.append(cmd(xvel=0.5 * kcfg.vx_hi, yvel=0.5 * kcfg.vy_hi, yawrate=0.5 * kcfg.wz_hi))
    grid.append(cmd(baseheight=0.5 * kcfg.bh_lo, baseroll=0.5 * kcfg.rx_hi, basepitch=0.5 * kcfg.ry_hi))
    return grid


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
    cfg = task.config
    commands = default_command_grid(task.kcfg) if commands is None else commands
    table = command_table(commands)
    if len(commands) == 0 or repeats < 1:
        raise ValueError("tracking_sweep needs at least one command and one repeat")
    ncmd, n = len(commands), len(commands) * repeats
    T = max(1, int(round((cfg.render_length_seconds if seconds is None else seconds) / cfg.ctrl_dt)))
    steps = settle_steps(cfg.tracking_settle_seconds if settle_seconds is None else settle_seconds, cfg.ctrl_dt)
    dev = task.device
    per_env = torch.from_numpy(np.tile(table, (repeats, 1))).to(dev)                      # env e follows command e % ncmd
    with held_command_rollout(task, n, T, ScriptedCommand(per_env), seed_offset) as (ctx, tr):
        err = torch.empty(T, n, R["SIZE"], device=dev)
        stats = fresh_tracking_stats(ctx, tr.c, n, steps, dev, err)
        ctx.synchronize()
        e, done, vec = err.cpu().numpy().astype(np.float64), tr.done.cpu().numpy(), stats.cpu().numpy()
    settled = e[:, :, R["SETTLED"]] != 0
    out = []
    for i in range(ncmd):
        envs = range(i, n, ncmd)
        entry = dict(command=tuple(float(x) for x in table[i]), mode=constants.COMMAND_MODE_NAMES[command_mode(table[i])])
        for k, name in enumerate(constants.TRACKING_ERROR_NAMES):      # per env the mean over its settled rows, then the mean over the repeats that have any
            means = [e[settled[:, j], j, k].mean() for j in envs if settled[:, j].any()]
            entry[name] = float(np.mean(means)) if means else float("nan")
        entry["settled_rows"] = int(sum(settled[:, j].sum() for j in envs))
        entry["failures_per_s"] = failures_per_s(done, envs, repeats * T * cfg.ctrl_dt)
        out.append(entry)
    return out, SweepRecord(tr.aux, err, vec)


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
