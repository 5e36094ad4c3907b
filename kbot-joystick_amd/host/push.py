"""Scripted pushes and the push-recovery sweep: the Event term that applies one scheduled push per env (kbj_env_set_push through
UserTerms.apply_events), the rotation of a push direction into the robot's heading, the sweep behind HumanoidWalkingTask.push_sweep
(kbj_tracking_stats' per-row errors, then kbj_push_recovery with one group per case) and its table."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ..spec import constants, layout as L
from . import binding as B
from .sweep import case_envs, command_table, steps_of, sweep_rollout, sweep_terms
from .tracking import TrackingStats
from .traj_view import PushRequest

P, S, O = L.PREC, L.PSTAT, L.POUT

# The "back on the command" test of the sweep, per tracking error (constants.TRACKING_ERROR_NAMES; kbj_push_criteria.tol). These are SETTINGS,
# echoed in every entry - round figures of the size of the reward stack's error scales, not thresholds measured on any policy: 0.3 m/s,
# 0.5 rad/s, a tilt error of 0.03 (about 20 degrees), 5 cm of height; the arms are ignored.
DEFAULT_TOLERANCES = dict(lin_vel_err=0.3, yaw_rate_err=0.5, tilt_err=0.03, height_err=0.05, arm_sq_err=math.inf)


def heading_rotate(base_quat: torch.Tensor, vec: torch.Tensor) -> torch.Tensor:
    """vec [N, 3] given in the robot's heading frame (x forward, y left, z up) -> world frame: the rotation about z by the yaw of base_quat
    [N, 4] (w first). The yaw's cosine and sine are (1 - 2 (y^2 + z^2), 2 (w z + x y)) normalised, as the env kernel's feet observation takes
    them - no trigonometry; a base pointing straight up or down (both zero) counts as yaw 0."""
    w, x, y, z = base_quat.unbind(-1)
    sn, cs = 2 * (w * z + x * y), 1 - 2 * (y * y + z * z)
    h = torch.sqrt(sn * sn + cs * cs)
    ok = h > 0
    c, s = torch.where(ok, cs / h, torch.ones_like(h)), torch.where(ok, sn / h, torch.zeros_like(h))
    return torch.stack([c * vec[:, 0] - s * vec[:, 1], s * vec[:, 0] + c * vec[:, 1], vec[:, 2]], dim=-1)


class ScriptedPush:
    """An Event term (host/user_terms.py apply_events) that applies ONE scheduled push per env and keeps the built-in push event quiet:
    on row 0 and on the rows where an env's episode starts it writes next = PUSH_NEVER (an in-step reset re-arms the built-in schedule); on
    row `push_row` it writes every env's wrench - `local` [N, 6], force then torque in the robot's heading frame at that row, rotated into
    the world by the yaw of the row's base quaternion on the device - for `steps` [N] control steps. Its event state is one flag per env:
    0 until the env's built-in schedule has been switched off."""

    def __init__(self, local: torch.Tensor, steps: torch.Tensor, push_row: int):
        self.local, self.steps, self.push_row = local.to(torch.float32), steps.to(torch.float32), int(push_row)

    def initial_event_state(self, state, curriculum_level, rng):
        return torch.zeros(state.N, device=self.local.device)

    def __call__(self, state, event_state, curriculum_level, rng):
        n, dev = state.N, self.local.device
        never = torch.full((n,), L.PUSH_NEVER, device=dev)
        if state.row == self.push_row:
            wrench = torch.cat([heading_rotate(state.base_quat, self.local[:, :3]), heading_rotate(state.base_quat, self.local[:, 3:])], dim=1)
            return PushRequest(torch.ones(n, dtype=torch.bool, device=dev), wrench, self.steps, never), torch.ones_like(event_state)
        return PushRequest(event_state == 0, torch.zeros(n, 6, device=dev), torch.zeros(n, device=dev), never), torch.ones_like(event_state)


@dataclasses.dataclass
class PushRecord:
    """What a push sweep left on the device, for whoever wants more than the table: the aux rows [T + 1, N, AUX SIZE], kbj_tracking_stats'
    per-row output [T, N, TERR SIZE], kbj_push_recovery's rows [N, PREC SIZE] and group statistics [cases, PSTAT SIZE] (float64), the schedule
    [N, 2] int32; env n belongs to case n % cases. `push_state` (numpy [N, 8]): the push block of the env state (wrench, PUSH_REM, PUSH_NXT)
    read back after the last step."""
    aux: torch.Tensor
    err: torch.Tensor
    rec: torch.Tensor
    stats: torch.Tensor
    sched: torch.Tensor
    push_state: np.ndarray = None


def push_sweep(task, forces=(50.0, 100.0, 150.0, 200.0), directions_deg=(0, 45, 90, 135, 180, 225, 270, 315), duration: float = 0.2, command=None,
               push_at: float = 2.0, window: float = 3.0, hold: float = 0.5, tolerances=None, repeats: int = 4, torque=None, seed_offset: int = 7919):
    """The sweep behind HumanoidWalkingTask.push_sweep (see there): returns (entries, record) - one entry per (force, direction) case, and the
    PushRecord of what the run left on the device. Every call builds a context of its own and closes it again (host/sweep.py sweep_rollout)."""
    cfg = task.config
    forces, directions_deg = [float(f) for f in forces], [float(a) for a in directions_deg]
    cases = [(f, a) for f in forces for a in directions_deg]
    if not cases or repeats < 1:
        raise ValueError("push_sweep needs at least one force, one direction and one repeat")
    tol = dict(DEFAULT_TOLERANCES)
    tol.update(tolerances or {})
    if set(tol) != set(constants.TRACKING_ERROR_NAMES):
        raise ValueError(f"push_sweep: tolerances are named {constants.TRACKING_ERROR_NAMES}, got {sorted(set(tol) - set(constants.TRACKING_ERROR_NAMES))}")
    cmd = command_table([() if command is None else command], "push_sweep: the command")[0]
    dt = cfg.ctrl_dt
    row, d, win, hld = steps_of(push_at, dt), steps_of(duration, dt), steps_of(window, dt), max(1, steps_of(hold, dt))
    if row < hld or d < 0 or win < 0:
        raise ValueError("push_sweep: push_at must leave room for the hold rows in front of the push; duration and window must not be negative")
    ncases, T = len(cases), row + d + win
    tq = np.zeros(3, np.float32) if torque is None else np.asarray(torque, np.float32).reshape(3)
    wrench = np.array([(f * math.cos(math.radians(a)), f * math.sin(math.radians(a)), 0.0, *tq) for f, a in cases], np.float32)
    n, group, (local,) = case_envs(task, ncases, repeats, f"push_sweep: {ncases} cases, kbj_push_recovery", wrench)      # env e runs case e % ncases
    dev = task.device
    event = ScriptedPush(local, torch.full((n,), float(d), device=dev), row)
    terms = sweep_terms(task, events={"scripted_push": event})
    hooks = [terms.apply_resets, terms.apply_events] + ([terms.observe_rows] if any(task.extra_obs) else [])
    T = max(1, T)

    def configure(vcfg):
        vcfg.command_mode, vcfg.enable_pushes = 1, 1                                      # one held command (resets write it too); the step kernel reads the event state
        for k in range(L.NCMD):
            vcfg.fixed_command[k] = float(cmd[k])

    with sweep_rollout(task, n, T, configure, terms, hooks, hooks, seed_offset) as (ctx, tr):
        err = torch.empty(T, n, L.TERR["SIZE"], device=dev)
        TrackingStats.fresh(ctx, tr.c, n, dev, 0, err=err)
        sched = torch.tensor([[row, d]] * n, dtype=torch.int32, device=dev)
        crit = B.PushCriteria((B.C.c_float * L.NTERR)(*[tol[k] for k in constants.TRACKING_ERROR_NAMES]), hld, win)
        rec = torch.empty(n, P["SIZE"], device=dev)
        stats = torch.empty(ncases, S["SIZE"], dtype=torch.float64, device=dev)
        ctx.push_recovery(tr.c, err, sched, crit, rec, group, ncases, stats)
        ctx.synchronize()
        st = stats.cpu().numpy()
        push_state = ctx.env_get_state()[1][:, L.ES["PUSH"]:L.ES["PUSH"] + 8].copy()
    settings = dict(duration=d * dt, push_at=row * dt, window=win * dt, hold=hld * dt, command=tuple(float(x) for x in cmd), torque=tuple(float(x) for x in tq),
                    tolerances=dict(tol), repeats=repeats)
    entries = [dict(force=f, direction_deg=a, **settings, **case_summary(st[i], dt)) for i, (f, a) in enumerate(cases)]
    return entries, PushRecord(tr.aux, err, rec, stats, sched, push_state)


def case_summary(vec, ctrl_dt: float) -> dict:
    """One KBJ_PSTAT vector (layout.PSTAT) as the figures of a table line: `valid` pushes (fell + recovered + unrecovered + censored) and the
    `void` count, each outcome's fraction of the valid pushes, mean and maximum recovery time in seconds over the recovered pushes, mean and
    maximum of the peak tilt error and of the peak linear-velocity error over the valid ones. A mean or maximum over nothing is nan."""
    vec = np.asarray(vec, np.float64)
    cnt = {name: int(vec[S["COUNT"] + k]) for k, name in enumerate(constants.PUSH_OUTCOME_NAMES)}
    valid = cnt["fell"] + cnt["recovered"] + cnt["unrecovered"] + cnt["censored"]
    nan = float("nan")
    out = dict(valid=valid, void=cnt["void"])
    for name in ("fell", "recovered", "unrecovered", "censored"):
        out[name + "_frac"] = cnt[name] / valid if valid else nan
    out["recovery_s_mean"] = float(vec[S["REC_SUM"]]) / cnt["recovered"] * ctrl_dt if cnt["recovered"] else nan
    out["recovery_s_max"] = float(vec[S["REC_MAX"]]) * ctrl_dt if cnt["recovered"] else nan
    for name, k in (("peak_tilt", P["PEAK_TILT"] - P["PEAK_LIN"]), ("peak_lin_vel_err", 0)):
        out[name + "_mean"] = float(vec[S["PEAK_SUM"] + k]) / valid if valid else nan
        out[name + "_max"] = float(vec[S["PEAK_MAX"] + k]) if valid else nan
    return out


def format_push_table(entries) -> str:
    """push_sweep's result as a text table: one line per (force, direction) case - valid pushes and voids, the outcome fractions of the valid
    ones, recovery time, peak tilt and peak linear-velocity error - under a line that echoes the settings."""
    cols = ("fell_frac", "recovered_frac", "unrecovered_frac", "censored_frac", "recovery_s_mean", "recovery_s_max", "peak_tilt_mean", "peak_tilt_max",
            "peak_lin_vel_err_mean", "peak_lin_vel_err_max")
    heads = ("fell", "recovered", "unrecov", "censored", "rec_s", "rec_s_max", "tilt", "tilt_max", "lin_err", "lin_max")
    lines = []
    if entries:
        x = entries[0]
        tol = " ".join(f"{k}<={v:g}" for k, v in x["tolerances"].items())
        lines.append(f"push {x['duration']:g} s at {x['push_at']:g} s, window {x['window']:g} s, hold {x['hold']:g} s, {x['repeats']} repeats; settings, not measured thresholds: {tol}")
    lines.append(f"{'force_N':>8s}  {'dir_deg':>7s}  {'valid':>5s}  {'void':>4s}" + "".join(f"  {h:>9s}" for h in heads))
    for x in entries:
        lines.append(f"{x['force']:8.1f}  {x['direction_deg']:7.1f}  {x['valid']:5d}  {x['void']:4d}" + "".join(f"  {x[c]:9.3f}" for c in cols))
    return "\n".join(lines)
