"""Actuator statistics on the device (kbj_actuator_stats; HumanoidWalkingTaskConfig.actuator_stats): the levels a row is held against, the per-env
carry rows that live next to the env state, the result vectors as whole-body logger scalars and as a per-joint table in N m, rad/s and W - and
the sweep, the actuator table: one line per scripted command, pooled from the per-env record of one call."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ..spec import constants, layout as L
from . import binding as B
from . import dist as dist_util
from .device_stats import DeviceStats
from .sweep import command_sweep, format_command_table, table_cell

V, J, A, E = L.ACT, L.AJNT, L.AACC, L.AENV
NAN = float("nan")

# The three defaults below are SETTINGS of this build, not figures from the reference: its metadata.json carries a soft_torque_limit per joint
# (kbj_model.tau_limit) and no speed limit at all, and nothing in it says from which share of the limit on a motor counts as loaded or how close
# to a joint stop is too close.
DEFAULT_TORQUE_LEVEL = 0.9          # share of kbj_model.tau_limit
DEFAULT_SPEED_LIMIT = None          # rad/s; None: no speed level (+inf: counts nothing)
DEFAULT_STOP_MARGIN_DEG = 2.0       # degrees inside kbj_model.dof_range


def actuator_levels(model, torque_level: float = DEFAULT_TORQUE_LEVEL, speed_limit=DEFAULT_SPEED_LIMIT, stop_margin_deg: float = DEFAULT_STOP_MARGIN_DEG) -> B.ActuatorLevels:
    """The kbj_actuator_levels of a robot (spec/constants.JOINT_NAMES order): tau_level = torque_level x model.tau_limit; vel_level = +inf
    unless `speed_limit` (rad/s) is given, as one float or as 20; pos_lo / pos_hi = model.dof_range[6 + u] moved inwards by `stop_margin_deg`
    (a range narrower than twice the margin collapses to its middle). The defaults are settings of this build, not figures from the
    reference, which gives no speed limit.
    With randomisers on an env's own torque limit can be as low as torque_limit_scale_low x tau_limit (train.py:1102: 0.5), and the aux
    record holds the torque AFTER that env's clip: a motor that sits on such a reduced limit below tau_level is NOT counted as at the torque
    level. The count says how often the nominal motor is loaded, not how often a randomised one saturates."""
    if not (torque_level > 0):
        raise ValueError("torque_level must be positive")
    if not (stop_margin_deg >= 0):
        raise ValueError("stop_margin_deg must not be negative")
    lv = B.ActuatorLevels()
    vel = np.full(L.NU, np.inf) if speed_limit is None else np.asarray(speed_limit, np.float64).reshape(-1)
    if vel.size == 1:
        vel = np.full(L.NU, vel[0])
    if vel.size != L.NU:
        raise ValueError(f"speed_limit must be one float or {L.NU}")
    if not (vel > 0).all():
        raise ValueError("speed_limit must be positive")
    margin = math.radians(stop_margin_deg)
    for u in range(L.NU):
        lo, hi = float(model.dof_range[6 + u][0]) + margin, float(model.dof_range[6 + u][1]) - margin
        if lo > hi:
            lo = hi = 0.5 * (lo + hi)
        lv.tau_level[u], lv.vel_level[u], lv.pos_lo[u], lv.pos_hi[u] = torque_level * float(model.tau_limit[u]), vel[u], lo, hi
    return lv


def levels_of_config(model, config) -> B.ActuatorLevels:
    """actuator_levels from the three level settings of a HumanoidWalkingTaskConfig."""
    return actuator_levels(model, config.actuator_torque_level, config.actuator_speed_limit, config.actuator_stop_margin_deg)


def _joint_blocks(vec, mode=None) -> tuple:
    """(head [5+], joints [NU, AJNT SIZE]) of mode block `mode` of a KBJ_ACT vector - or, with mode None, of all modes together: counts and
    sums added, maxima taken."""
    vec = np.asarray(vec, np.float64)
    blocks = vec[:V["EPISODES"]].reshape(L.CMODE["COUNT"], V["MODE_STRIDE"])
    if mode is not None:
        b = blocks[mode]
    else:
        b = blocks.sum(0)
        for u in range(L.NU):
            for k in L.AJNT_MAX:
                s = V["JOINT"] + J["SIZE"] * u + J[k]
                b[s] = blocks[:, s].max()
    return b[:V["JOINT"]], b[V["JOINT"]:V["JOINT"] + L.NU * J["SIZE"]].reshape(L.NU, J["SIZE"])


def _div(a, b) -> float:
    return float(a) / float(b) if b > 0 else NAN


def _whole_body(head, joints, model, dt: float, tau_level) -> dict:
    """The whole-body figures of one (head, joints) block with rows."""
    rows, pairs, speed = float(head[V["ROWS"]]), float(head[V["PAIRS"]]), float(head[V["SPEED_SUM"]])
    pabs = float(joints[:, J["POW_ABS"]].sum())
    weight = float(model.total_mass) * math.sqrt(sum(float(g) ** 2 for g in model.gravity))
    frac = joints[:, J["TAU_MAX"]] / np.asarray(tau_level, np.float64)
    worst = int(np.argmax(frac))
    return dict(power_abs_w=pabs / rows, power_pos_w=float(joints[:, J["POW_POS"]].sum()) / rows,
                # both sums carry the same dt (J = W x dt, m = m/s x dt): it cancels
                cost_of_transport=pabs / (weight * speed) if speed * dt >= 0.1 else NAN,
                torque_rms=math.sqrt(float(joints[:, J["TAU_SQ"]].sum()) / (rows * L.NU)),
                at_torque_level_frac=float(head[V["ANY_TAU_ROWS"]]) / rows, at_stop_frac=float(head[V["ANY_STOP_ROWS"]]) / rows,
                action_rate_rms=math.sqrt(_div(joints[:, J["DACT_SQ"]].sum(), pairs * L.NU)), action_rate_max=float(joints[:, J["DACT_MAX"]].max()) if pairs > 0 else NAN,
                worst_joint=float(worst), worst_joint_frac=float(frac[worst]))


def actuator_scalars(vec, model, dt: float, prefix: str = "act/", levels=None) -> dict:
    """One KBJ_ACT vector (kbj_model.h; layout.ACT / AJNT) as logger scalars: whole-body figures only, about ten per mode and not a thousand
    (the per-joint figures: actuator_joint_table). Per mode that has rows, `<prefix><mode>/...`: power_abs_w and power_pos_w (the mean over
    rows of the sum over joints of |P| and of max(P, 0); P is the control-rate estimate kbj.h defines); cost_of_transport = sum |P| /
    (total_mass x |g| x sum speed), nan where the mode's rows covered less than 0.1 m; torque_rms (N m, over rows and joints);
    at_torque_level_frac and at_stop_frac (rows with at least one joint there); action_rate_rms and action_rate_max (rad per control step,
    over the rows with a previous row in the same episode; nan without any); worst_joint, the index (spec/constants.JOINT_NAMES) of the
    largest TAU_MAX / tau_level, and worst_joint_frac. `levels`: the ActuatorLevels the vector was taken with (default: actuator_levels(model))."""
    lv = actuator_levels(model) if levels is None else levels
    out = {}
    for m, mode in enumerate(constants.COMMAND_MODE_NAMES):
        head, joints = _joint_blocks(vec, m)
        if head[V["ROWS"]] <= 0:
            continue
        for k, x in _whole_body(head, joints, model, dt, list(lv.tau_level)).items():
            out[f"{prefix}{mode}/{k}"] = x
    return out


def actuator_joint_table(vec, model, dt: float, mode=None) -> list:
    """One KBJ_ACT vector per joint: a dict per actuator, by name - torque_rms_frac and torque_max_frac (as a fraction of model.tau_limit),
    torque_level_frac (share of rows at the torque level), speed_rms and speed_max (rad/s), power_abs_w (mean |P|) and power_max_w,
    stop_frac (share of rows at a joint stop), action_rate_rms (rad per control step) and action_rate_rms_per_s (rad/s). `mode`: a
    command mode's index, or None for all rows together. nan over nothing."""
    head, joints = _joint_blocks(vec, mode)
    rows, pairs = float(head[V["ROWS"]]), float(head[V["PAIRS"]])
    out = []
    for u, name in enumerate(constants.JOINT_NAMES):
        x, lim = joints[u], float(model.tau_limit[u])
        rate = math.sqrt(_div(x[J["DACT_SQ"]], pairs))
        out.append(dict(joint=name, torque_rms_frac=math.sqrt(_div(x[J["TAU_SQ"]], rows)) / lim, torque_max_frac=(float(x[J["TAU_MAX"]]) / lim) if rows > 0 else NAN,
                        torque_level_frac=_div(x[J["TAU_ROWS"]], rows), speed_rms=math.sqrt(_div(x[J["VEL_SQ"]], rows)), speed_max=float(x[J["VEL_MAX"]]) if rows > 0 else NAN,
                        power_abs_w=_div(x[J["POW_ABS"]], rows), power_max_w=float(x[J["POW_MAX"]]) if rows > 0 else NAN, stop_frac=_div(x[J["STOP_ROWS"]], rows),
                        action_rate_rms=rate, action_rate_rms_per_s=rate / dt))
    return out


JOINT_TABLE_COLUMNS = (("tau rms/lim", "torque_rms_frac"), ("tau max/lim", "torque_max_frac"), ("at level", "torque_level_frac"), ("w rms", "speed_rms"), ("w max", "speed_max"),
                       ("|P| mean W", "power_abs_w"), ("|P| peak W", "power_max_w"), ("at stop", "stop_frac"), ("da rms", "action_rate_rms"))


def format_actuator_joint_table(table) -> str:
    """actuator_joint_table's result as text: one line per joint ("-" where there was nothing to average)."""
    w = max([len("joint")] + [len(x["joint"]) for x in table])
    lines = [f"{'joint':{w}s}" + "".join(f"  {title:>10s}" for title, _ in JOINT_TABLE_COLUMNS)]
    for x in table:
        lines.append(f"{x['joint']:{w}s}" + "".join(table_cell(x[key]) for _, key in JOINT_TABLE_COLUMNS))
    return "\n".join(lines)


class ActuatorStats(DeviceStats):
    """kbj_actuator_stats over the rollouts of a run: every env's previous action and whether its episode runs (KBJ_AACC rows), the KBJ_ACT
    vectors of the last rollout's rows and of all so far. `levels`: what every call is held against. `model`, `ctrl_dt`: what `scalars`
    turns a vector into watts and a cost of transport with."""
    layout, acc_width, acc_key, total_key = dist_util.ACTUATOR_STATS, A["SIZE"], "act_acc", "act_total"
    switch, prefix, total_prefix, valid_prefix = "actuator_stats", "act/", "act_total/", "valid/act/"

    def __init__(self, num_envs: int, levels: B.ActuatorLevels, device, model=None, ctrl_dt=None):
        self.levels, self.settings, self.model, self.ctrl_dt = levels, (levels,), model, ctrl_dt
        super().__init__(num_envs, device)

    @staticmethod
    def call(ctx, traj, acc, stats, levels, env=None):
        ctx.actuator_stats(traj, levels, acc, stats, env)

    def scalars(self, vec, prefix: str) -> dict:
        return actuator_scalars(vec, self.model, self.ctrl_dt, prefix, self.levels)


# ---- the sweep ----
@dataclasses.dataclass
class ActuatorRecord:
    """What an actuator sweep left on the device, for whoever wants more than the table: the aux rows [T + 1, N, AUX SIZE], the state record
    [T, N, QSTATE SIZE], the actions [T, N, 20] and the per-env record [N, AENV SIZE] of kbj_actuator_stats; env n follows command
    n % len(commands). `stats` is the call's KBJ_ACT vector, `levels` what it was held against."""
    aux: torch.Tensor
    qstate: torch.Tensor
    action: torch.Tensor
    env: torch.Tensor
    stats: np.ndarray
    levels: B.ActuatorLevels


def pool_actuator_rows(rows, model, dt: float) -> dict:
    """Actuator figures of several envs together, from their KBJ_AENV rows [k, AENV SIZE]: counts and sums add up in float64; the joint
    nearest its level is the PEAK_JOINT of the env with the largest PEAK_FRAC (the first such env); nan where there is nothing to divide by."""
    r = np.asarray(rows, np.float64).reshape(-1, E["SIZE"])
    tot = r.sum(0)
    n, pairs, speed = tot[E["ROWS"]], tot[E["PAIRS"]], tot[E["SPEED_SUM"]]
    weight = float(model.total_mass) * math.sqrt(sum(float(g) ** 2 for g in model.gravity))
    top = int(np.argmax(r[:, E["PEAK_FRAC"]])) if len(r) else -1
    joint = int(r[top, E["PEAK_JOINT"]]) if top >= 0 else -1
    return dict(power_abs_w=_div(tot[E["POW_ABS"]], n), power_pos_w=_div(tot[E["POW_POS"]], n),
                cost_of_transport=float(tot[E["POW_ABS"]]) / (weight * float(speed)) if speed * dt >= 0.1 else NAN,
                torque_rms=math.sqrt(_div(tot[E["TAU_SQ"]], n * L.NU)), at_torque_level_frac=_div(tot[E["ANY_TAU_ROWS"]], n), at_stop_frac=_div(tot[E["ANY_STOP_ROWS"]], n),
                action_rate_rms=math.sqrt(_div(tot[E["DACT_SQ"]], pairs * L.NU)),
                worst_joint=constants.JOINT_NAMES[joint] if joint >= 0 else "-", worst_joint_frac=float(r[top, E["PEAK_FRAC"]]) if joint >= 0 else NAN)


def actuator_sweep(task, commands=None, repeats: int = 2, seconds=None, seed_offset: int = 7919, **levels):
    """The sweep behind HumanoidWalkingTask.actuator_sweep (see there): returns (entries, record) - one entry per command, and the
    ActuatorRecord of what the run left on the device. The rollout is tracking_sweep's (host/sweep.py held_command_rollout under a
    ScriptedCommand term) with the state record kept; one kbj_actuator_stats call on a fresh carry then gives every env's totals. `levels`:
    keyword arguments of actuator_levels (default: the task config's three level settings). Like the gait and push tables, this one has
    NOT been taken on a trained policy: what a policy fit for the robot looks like in it is not known from this build."""
    cfg, dev = task.config, task.device
    lv = actuator_levels(task.model_blob, **levels) if levels else levels_of_config(task.model_blob, cfg)
    with command_sweep(task, "actuator_sweep", commands, repeats, seconds, seed_offset, record_state=True) as (ctx, tr, n, T, entries):
        env = torch.empty(n, E["SIZE"], device=dev)
        stats = ActuatorStats.fresh(ctx, tr.c, n, dev, lv, env=env)
        ctx.synchronize()
        rows, vec = env.cpu().numpy(), stats.cpu().numpy()
    return entries(lambda envs: pool_actuator_rows(rows[envs], task.model_blob, cfg.ctrl_dt)), ActuatorRecord(tr.aux, tr.qstate, tr.action, env, vec, lv)


ACTUATOR_TABLE_COLUMNS = (("|P| W", "power_abs_w"), ("P+ W", "power_pos_w"), ("CoT", "cost_of_transport"), ("torque rms", "torque_rms"), ("at level", "at_torque_level_frac"),
                          ("at stop", "at_stop_frac"), ("da rms", "action_rate_rms"), ("worst frac", "worst_joint_frac"), ("fail/s", "failures_per_s"))


def format_actuator_table(entries) -> str:
    """actuator_sweep's result as a text table: one line per command (its non-zero components by name), then mean |P| and mean positive
    power, the cost of transport, the torque level, the shares of rows with a joint at its torque level and at a stop, the action rate, the
    joint nearest its torque level by fraction and name, and the failures per second ("-" where there was nothing to average)."""
    return format_command_table(entries, ACTUATOR_TABLE_COLUMNS, last=("worst joint", "worst_joint"))
