"""The command step response and its sweep: the Command term that changes every env's command once, on a scheduled row
(SteppedCommand), the default transitions, the sweep behind HumanoidWalkingTask.step_sweep (one rollout, then ONE kbj_step_response call with
one group per transition) and its table. The rule is in include/kbj.h at kbj_step_response."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from ..spec import constants, layout as L
from . import binding as B
from .sweep import case_envs, command_label, command_table, held_command_rollout, steps_of, table_cell

R, S, O = L.SREC, L.SSTAT, L.SOUT
CHANNELS = constants.STEP_CHANNEL_NAMES
MAX_SMOOTH_ROWS = 32          # kbj_step_criteria.smooth_steps: the rows of the kernel's smoothing ring


class SteppedCommand:
    """A Command term (train.py:724, 768) that changes every env's command ONCE: on the rows before `step_row` an env holds its row of
    `table0` [N, 16], from `step_row` on its row of `table1`. Both `initial_command` and `__call__` answer by the row alone, so the
    schedule survives an in-episode reset, after which the kernel's own reset (command_mode = 1) has returned the env to the context's
    single fixed_command - as ScriptedCommand's does."""

    def __init__(self, table0: torch.Tensor, table1: torch.Tensor, step_row: int):
        self.table0, self.table1, self.step_row = table0.to(torch.float32), table1.to(torch.float32), int(step_row)

    def scheduled(self, state):
        return self.table0 if state.row < self.step_row else self.table1

    def initial_command(self, state, curriculum_level, rng):
        return self.scheduled(state)

    def __call__(self, prev_command, state, curriculum_level, rng):
        return self.scheduled(state)


def default_step_grid(kcfg) -> list:
    """The sweep's default transitions (from, to), from the command ranges of a kbj_config (train.py:1211-1217): stand -> forward full
    (vx_hi) and back (the stop); stand -> backward full (vx_lo); stand -> left full (vy_hi) and back; stand -> turn-left full (wz_hi) and
    back; forward half -> forward full; forward full -> backward full (the reversal); turn-left full -> turn-right full (wz_lo). 10 pairs
    of 16 floats, pose and arms at zero."""
    def cmd(**kw):
        c = [0.0] * L.NCMD
        for k, v in kw.items():
            c[constants.COMMAND_NAMES.index(k)] = float(v)
        return tuple(c)
    stand, fwd, back = cmd(), cmd(xvel=kcfg.vx_hi), cmd(xvel=kcfg.vx_lo)
    left, turn_l, turn_r = cmd(yvel=kcfg.vy_hi), cmd(yawrate=kcfg.wz_hi), cmd(yawrate=kcfg.wz_lo)
    return [(stand, fwd), (fwd, stand), (stand, back), (stand, left), (left, stand), (stand, turn_l), (turn_l, stand),
            (cmd(xvel=0.5 * kcfg.vx_hi), fwd), (fwd, back), (turn_l, turn_r)]


@dataclasses.dataclass
class StepRecord:
    """What a step sweep left on the device, for whoever wants more than the table: the aux rows [T + 1, N, AUX SIZE], kbj_step_response's
    signal [T, N, SSIG SIZE], its records [N, SREC SIZE] and group statistics [cases, SSTAT SIZE] (float64), the schedule [N] int32; env n
    belongs to case n % cases."""
    aux: torch.Tensor
    sig: torch.Tensor
    rec: torch.Tensor
    stats: torch.Tensor
    sched: torch.Tensor


def step_sweep(task, transitions=None, step_at: float = 3.0, window: float = 4.0, hold: float = 0.5, smooth: float = 0.5, rise_level: float = 0.9,
               band_frac: float = 0.1, band_abs=(0.15, 0.15, 0.25), min_step=(0.05, 0.05, 0.05), repeats: int = 4, seed_offset: int = 7919):
    """The sweep behind HumanoidWalkingTask.step_sweep (see there): returns (entries, record) - one entry per transition, and the StepRecord
    of what the run left on the device. Every call builds a context of its own and closes it again (host/sweep.py sweep_rollout)."""
    cfg = task.config
    transitions = default_step_grid(task.kcfg) if transitions is None else list(transitions)
    if not transitions or repeats < 1:
        raise ValueError("step_sweep needs at least one transition and one repeat")
    if any(len(tr) != 2 for tr in transitions):
        raise ValueError("step_sweep: a transition is a pair (from command, to command)")
    t0, t1 = (command_table([tr[k] for tr in transitions], "step_sweep: the " + end + " command of transition {i}") for k, end in enumerate(("from", "to")))
    dt = cfg.ctrl_dt
    row, win, hld, m = steps_of(step_at, dt), steps_of(window, dt), max(1, steps_of(hold, dt)), max(1, steps_of(smooth, dt))
    if m > MAX_SMOOTH_ROWS:
        raise ValueError(f"step_sweep: smooth = {smooth:g} s is {m} rows at ctrl_dt = {dt:g} s; kbj_step_response smooths over at most {MAX_SMOOTH_ROWS} rows "
                         f"(the kernel keeps that many rows of the signal per env)")
    if row < hld or win < 1:
        raise ValueError("step_sweep: step_at must leave room for the hold rows in front of the step, and window must be at least one row")
    band_abs, min_step = [float(x) for x in band_abs], [float(x) for x in min_step]
    if len(band_abs) != L.NSCH or len(min_step) != L.NSCH:
        raise ValueError(f"step_sweep: band_abs and min_step have one value per channel {CHANNELS}")
    ncases, T = len(transitions), row + win
    n, group, (per_env0, per_env1) = case_envs(task, ncases, repeats, f"step_sweep: {ncases} transitions, kbj_step_response", t0, t1)      # env e runs case e % ncases
    dev = task.device
    with held_command_rollout(task, n, T, SteppedCommand(per_env0, per_env1, row), seed_offset) as (ctx, tr):
        sched = torch.full((n,), row, dtype=torch.int32, device=dev)
        crit = B.StepCriteria((B.C.c_float * L.NSCH)(*min_step), (B.C.c_float * L.NSCH)(*band_abs), band_frac, rise_level, m, hld, win)
        sig = torch.empty(T, n, L.SSIG["SIZE"], device=dev)
        rec = torch.empty(n, R["SIZE"], device=dev)
        stats = torch.empty(ncases, S["SIZE"], dtype=torch.float64, device=dev)
        ctx.step_response(tr.c, sched, crit, sig, rec, group, ncases, stats)
        ctx.synchronize()
        st = stats.cpu().numpy()
    settings = dict(step_at=row * dt, window=win * dt, hold=hld * dt, smooth=m * dt, rise_level=float(rise_level), band_frac=float(band_frac),
                    band_abs=tuple(band_abs), min_step=tuple(min_step), repeats=repeats)
    entries = [dict(from_command=tuple(float(x) for x in t0[i]), to_command=tuple(float(x) for x in t1[i]), **settings, **case_summary(st[i], dt))
               for i in range(ncases)]
    return entries, StepRecord(tr.aux, sig, rec, stats, sched)


def case_summary(vec, ctrl_dt: float) -> dict:
    """One KBJ_SSTAT vector (layout.SSTAT) as the figures of a table line: `valid` steps (fell + settled + unsettled + censored) and the
    `void` count, each outcome's fraction of the valid ones, mean and maximum settling time and mean time to the fall in seconds; per channel
    (constants.STEP_CHANNEL_NAMES) `<ch>_active` envs, the share of them that reached the rise level (`_risen_frac`), mean and maximum rise
    time in seconds, mean and maximum overshoot, mean and maximum cross-coupling over the envs where the channel did not move
    (`_coupling_`; m/s, m/s, rad/s), and over the settled envs the mean signed travel and its largest magnitude in metres (forward,
    sideways) and radians (yaw): the device's (m/s) x rows times ctrl_dt. A figure over nothing is nan."""
    vec = np.asarray(vec, np.float64)
    nan = float("nan")
    div = lambda a, b: float(a) / float(b) if b > 0 else nan
    cnt = {name: int(vec[S["COUNT"] + k]) for k, name in enumerate(constants.STEP_OUTCOME_NAMES)}
    valid = cnt["fell"] + cnt["settled"] + cnt["unsettled"] + cnt["censored"]
    out = dict(valid=valid, void=cnt["void"])
    for name in ("fell", "settled", "unsettled", "censored"):
        out[name + "_frac"] = div(cnt[name], valid)
    out["settle_s_mean"] = div(vec[S["SETTLE_SUM"]], cnt["settled"]) * ctrl_dt
    out["settle_s_max"] = float(vec[S["SETTLE_MAX"]]) * ctrl_dt if cnt["settled"] else nan
    out["fall_s_mean"] = div(vec[S["FALL_SUM"]], cnt["fell"]) * ctrl_dt
    for k, ch in enumerate(CHANNELS):
        active, risen, quiet = int(vec[S["ACTIVE_N"] + k]), int(vec[S["RISE_N"] + k]), int(vec[S["DEV_N"] + k])
        out[ch + "_active"] = active
        out[ch + "_risen_frac"] = div(risen, active)
        out[ch + "_rise_s_mean"] = div(vec[S["RISE_SUM"] + k], risen) * ctrl_dt
        out[ch + "_rise_s_max"] = float(vec[S["RISE_MAX"] + k]) * ctrl_dt if risen else nan
        out[ch + "_overshoot_mean"] = div(vec[S["OVER_SUM"] + k], active)
        out[ch + "_overshoot_max"] = float(vec[S["OVER_MAX"] + k]) if active else nan
        out[ch + "_coupling_mean"] = div(vec[S["DEV_SUM"] + k], quiet)
        out[ch + "_coupling_max"] = float(vec[S["DEV_MAX"] + k]) if quiet else nan
        out[ch + "_travel_mean"] = div(vec[S["TRAVEL_SUM"] + k], cnt["settled"]) * ctrl_dt
        out[ch + "_travel_absmax"] = float(vec[S["TRAVEL_ABSMAX"] + k]) * ctrl_dt if cnt["settled"] else nan
    return out


def format_step_table(entries) -> str:
    """step_sweep's result as a text table: one line per transition (the non-zero components of both commands by name) - valid steps and
    voids, the outcome fractions of the valid ones, settling time, then over the channels that moved the rise time, the risen share and
    the overshoot, over those that did not the cross-coupling, and the forward travel of the settled envs ("-" over nothing) - under a line
    that echoes the settings."""
    def pooled(x, key, how):                     # over the channels: the active ones for rise and overshoot, the quiet ones for the coupling
        vals = [x[f"{ch}_{key}"] for ch in CHANNELS]
        vals = [v for v in vals if v == v]
        return how(vals) if vals else float("nan")
    cols = (("fell", lambda x: x["fell_frac"]), ("settled", lambda x: x["settled_frac"]), ("unsettled", lambda x: x["unsettled_frac"]),
            ("censored", lambda x: x["censored_frac"]), ("settle_s", lambda x: x["settle_s_mean"]), ("settle_max", lambda x: x["settle_s_max"]),
            ("rise_s", lambda x: pooled(x, "rise_s_mean", max)), ("risen", lambda x: pooled(x, "risen_frac", min)),
            ("overshoot", lambda x: pooled(x, "overshoot_max", max)), ("coupling", lambda x: pooled(x, "coupling_max", max)),
            ("travel_m", lambda x: x["forward_travel_mean"]))
    lines = []
    if entries:
        x = entries[0]
        bands = " ".join(f"{ch}: band>={b:g} step>={s:g}" for ch, b, s in zip(CHANNELS, x["band_abs"], x["min_step"]))
        lines.append(f"step at {x['step_at']:g} s, window {x['window']:g} s, hold {x['hold']:g} s, smoothing {x['smooth']:g} s, {x['repeats']} repeats; settings, not measured "
                     f"thresholds: rise level {x['rise_level']:g}, band {x['band_frac']:g} of the step, {bands}")
    labels = [f"{command_label(x['from_command'])} -> {command_label(x['to_command'])}" for x in entries]
    w = max([len("transition")] + [len(s) for s in labels])
    lines.append(f"{'transition':{w}s}  {'valid':>5s}  {'void':>4s}" + "".join(f"  {title:>10s}" for title, _ in cols))
    for s, x in zip(labels, entries):
        lines.append(f"{s:{w}s}  {x['valid']:5d}  {x['void']:4d}" + "".join(table_cell(get(x)) for _, get in cols))
    return "\n".join(lines)
