"""Scripted model perturbations and the robustness sweep: what a policy does on a robot that is NOT the model it trained on. The Perturbation
a case names (friendly fields -> the KBJ_PERT record kbj_env_perturb takes), whether it lies inside what the built-in randomisers draw
(in_training_range), the sweep behind HumanoidWalkingTask.robustness_sweep (held commands under perturbed model rows, written again after
every in-episode reset; kbj_tracking_stats' per-row errors, then ONE kbj_robustness call with one group per case), what the host makes of
a group's statistics, and the table. The rules are in include/kbj.h at kbj_env_perturb and kbj_robustness."""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from ..spec import constants, layout as L
from . import binding as B
from .sweep import ScriptedCommand, case_envs, command_label, command_mode, command_table, held_command_rollout, steps_of, table_cell
from .tracking import TrackingStats, settle_steps

P, R, S = L.PERT, L.RREC, L.RSTAT
# the joints a per-joint field may name at once (constants.JOINT_NAMES order: left leg, right leg, right arm, left arm)
JOINT_GROUPS = dict(left_leg=range(0, 5), right_leg=range(5, 10), right_arm=range(10, 15), left_arm=range(15, 20))
_PER_JOINT = dict(kp_scale=("KP_SCALE", 1.0), kd_scale=("KD_SCALE", 1.0), torque_scale=("TAULIM_SCALE", 1.0), action_bias=("ACTBIAS", 0.0))


@dataclasses.dataclass
class Perturbation:
    """One way the robot differs from the model (kbj_model.h KBJ_PERT_*). Scales multiply the model's value, `payload_kg` is a point mass at the
    torso's centre of mass, `com_shift` metres added to it, `latency_substeps` the action latency in physics substeps (None keeps what each
    episode drew), `action_bias` radians. `kp_scale`, `kd_scale`, `torque_scale` and `action_bias` are a number for all joints or a dict
    whose keys are joint names (constants.JOINT_NAMES) or the groups left_leg, right_leg, right_arm, left_arm; joints a dict does not name
    keep the default, later keys win."""
    name: str = "nominal"
    mass_scale: float = 1.0
    payload_kg: float = 0.0
    friction_scale: float = 1.0
    armature_scale: float = 1.0
    frictionloss_scale: float = 1.0
    latency_substeps: Optional[int] = None
    com_shift: tuple = (0.0, 0.0, 0.0)
    kp_scale: object = 1.0
    kd_scale: object = 1.0
    torque_scale: object = 1.0
    action_bias: object = 0.0

    def per_joint(self, field: str) -> np.ndarray:
        """[20] float64: the per-joint field `field` spread over the joints. Raises ValueError naming the field on an unknown key."""
        value, default = getattr(self, field), _PER_JOINT[field][1]
        out = np.full(L.NU, default, np.float64)
        if isinstance(value, dict):
            for key, v in value.items():
                if key in JOINT_GROUPS:
                    out[list(JOINT_GROUPS[key])] = float(v)
                elif key in constants.JOINT_NAMES:
                    out[constants.JOINT_NAMES.index(key)] = float(v)
                else:
                    raise ValueError(f"Perturbation {self.name!r}: {field} names {key!r}, which is neither a joint (constants.JOINT_NAMES) nor one of {sorted(JOINT_GROUPS)}")
        else:
            out[:] = float(value)
        return out

    def record(self) -> np.ndarray:
        """The [PERT SIZE] float32 record kbj_env_perturb takes. Everything the kernel would refuse is refused here, by field, with a
        ValueError - before any device is touched."""
        def bad(field, why):
            return ValueError(f"Perturbation {self.name!r}: {field} {why}")
        rec = np.zeros(P["SIZE"], np.float32)
        for field, slot, positive in (("mass_scale", "MASS_SCALE", True), ("payload_kg", "PAYLOAD", False), ("friction_scale", "MU_SCALE", True),
                                      ("armature_scale", "ARMATURE_SCALE", True), ("frictionloss_scale", "FRICLOSS_SCALE", False)):
            v = float(getattr(self, field))
            if not math.isfinite(v) or (v <= 0 if positive else v < 0):
                raise bad(field, f"= {v!r} must be finite and {'positive' if positive else 'not negative'}")
            rec[P[slot]] = v
        lat = self.latency_substeps
        if lat is None:
            rec[P["LATENCY"]] = -1.0
        else:
            if isinstance(lat, bool) or not math.isfinite(float(lat)) or float(lat) != math.floor(float(lat)) or float(lat) < 0:
                raise bad("latency_substeps", f"= {lat!r} must be None (keep) or a whole number of substeps that is not negative")
            rec[P["LATENCY"]] = float(lat)
        shift = np.asarray(self.com_shift, np.float64).reshape(-1)
        if shift.shape != (3,) or not np.isfinite(shift).all():
            raise bad("com_shift", f"= {self.com_shift!r} must be three finite metres")
        rec[P["COM_SHIFT"]:P["COM_SHIFT"] + 3] = shift
        for field, (slot, _) in _PER_JOINT.items():
            v = self.per_joint(field)
            if not np.isfinite(v).all():
                raise bad(field, "must be finite")
            if field in ("kp_scale", "torque_scale") and (v <= 0).any():
                raise bad(field, "must be positive")
            if field == "kd_scale" and (v < 0).any():
                raise bad(field, "must not be negative")
            rec[P[slot]:P[slot] + L.NU] = v
        return rec

    def changed(self) -> dict:
        """The fields that differ from the nominal model, as given."""
        nominal = Perturbation()
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self) if f.name != "name" and getattr(self, f.name) != getattr(nominal, f.name)}


def latency_range(kcfg) -> tuple[int, int]:
    """(lowest, highest) action latency in substeps that the reset path draws from a kbj_config: floor(u / dt + 0.5) for u uniform in
    [latency_lo, latency_hi), in the kernel's fp32 arithmetic."""
    lo, hi = (float(np.float32(x) / np.float32(kcfg.dt)) for x in (kcfg.latency_lo, kcfg.latency_hi))
    return int(math.floor(lo + 0.5)), max(int(math.floor(lo + 0.5)), int(math.ceil(hi + 0.5)) - 1)


def in_training_range(perturbation: Perturbation, kcfg) -> bool:
    """Whether every knob of `perturbation` lies inside what the built-in randomisers of the kbj_config `kcfg` (task.kcfg) draw at a reset
    (csrc/kbj_env_task.h task_randomize): mass within 1 +- inertia_scale, kp and kd within [1 / scale, scale], torque within
    [torque_limit_scale_low, 1], armature and frictionloss within their ranges, the latency among the substeps latency_lo .. latency_hi give
    (None: kept, inside), every action bias within +- action_bias_scale, every COM shift component within +- com_jitter. The friction is
    never randomised and no payload is ever drawn: only friction x 1 and 0 kg are inside. With enable_randomizers off the policy has
    seen the nominal model alone: anything that differs from it is outside (a latency is still compared with the drawn range)."""
    p, rec = perturbation, perturbation.record()
    lat_ok = p.latency_substeps is None or latency_range(kcfg)[0] <= int(p.latency_substeps) <= latency_range(kcfg)[1]
    if not kcfg.enable_randomizers:
        nominal = Perturbation(latency_substeps=p.latency_substeps).record()
        return lat_ok and bool(np.array_equal(rec, nominal))
    within = lambda v, lo, hi: bool((np.asarray(v, np.float64) >= float(lo)).all() and (np.asarray(v, np.float64) <= float(hi)).all())
    f = lambda x: float(np.float32(x))
    joint = lambda slot: rec[P[slot]:P[slot] + L.NU]
    return (lat_ok and within(rec[P["MASS_SCALE"]], 1 - f(kcfg.inertia_scale), 1 + f(kcfg.inertia_scale)) and rec[P["PAYLOAD"]] == 0 and rec[P["MU_SCALE"]] == 1
            and within(rec[P["ARMATURE_SCALE"]], f(kcfg.armature_scale_lo), f(kcfg.armature_scale_hi))
            and within(rec[P["FRICLOSS_SCALE"]], f(kcfg.fricloss_scale_lo), f(kcfg.fricloss_scale_hi))
            and within(joint("KP_SCALE"), 1.0 / f(kcfg.kp_scale), f(kcfg.kp_scale)) and within(joint("KD_SCALE"), 1.0 / f(kcfg.kd_scale), f(kcfg.kd_scale))
            and within(joint("TAULIM_SCALE"), f(kcfg.torque_limit_scale_low), 1.0)
            and within(joint("ACTBIAS"), -f(kcfg.action_bias_scale), f(kcfg.action_bias_scale))
            and within(rec[P["COM_SHIFT"]:P["COM_SHIFT"] + 3], -f(kcfg.com_jitter), f(kcfg.com_jitter)))


def default_perturbations() -> list:
    """The sweep's default cases. SETTINGS of this build - round figures around and beyond the randomisers' ranges - not thresholds measured
    on any policy."""
    Pn = Perturbation
    return [Pn("nominal"), Pn("friction x0.5", friction_scale=0.5), Pn("friction x0.25", friction_scale=0.25), Pn("mass x0.85", mass_scale=0.85),
            Pn("mass x1.15", mass_scale=1.15), Pn("payload 5 kg", payload_kg=5.0), Pn("kp x0.7", kp_scale=0.7), Pn("kp x1.3", kp_scale=1.3), Pn("kd x0.5", kd_scale=0.5),
            Pn("torque x0.7", torque_scale=0.7), Pn("torque x0.5", torque_scale=0.5), Pn("latency 0", latency_substeps=0), Pn("latency 5", latency_substeps=5),
            Pn("armature x2", armature_scale=2.0), Pn("frictionloss x3", frictionloss_scale=3.0), Pn("left leg torque x0.6", torque_scale={"left_leg": 0.6})]


def default_robustness_commands(kcfg) -> list:
    """The sweep's default commands, from the command ranges of a kbj_config: stand, forward at half and at full range, turn left at full range."""
    cmd = lambda **kw: tuple(float(kw.get(name, 0.0)) for name in constants.COMMAND_NAMES)
    return [cmd(), cmd(xvel=0.5 * kcfg.vx_hi), cmd(xvel=kcfg.vx_hi), cmd(yawrate=kcfg.wz_hi)]


@dataclasses.dataclass
class RobustnessRecord:
    """What a robustness sweep left behind, for whoever wants more than the table: the aux rows [T + 1, N, AUX SIZE], kbj_tracking_stats'
    per-row output [T, N, TERR SIZE], kbj_robustness' records [N, RREC SIZE] and group statistics [cases, RSTAT SIZE] (both float64), the
    group of every env [N] int32 (env n runs case n % cases), the perturbation record of every env [N, PERT SIZE], and `ep` (numpy
    [N, EP SIZE]): the model rows read back after the last step."""
    aux: torch.Tensor
    err: torch.Tensor
    rec: torch.Tensor
    stats: torch.Tensor
    group: torch.Tensor
    pert: torch.Tensor
    ep: np.ndarray


def case_summary(vec, ctrl_dt: float) -> dict:
    """One KBJ_RSTAT vector (layout.RSTAT) as the figures of a table line: `envs`; `survival`, the share of them that never fell;
    `falls_per_s` over the seconds the envs ran together; `first_fall_s_mean` / `first_fall_s_min` over the envs that fell; `timeouts`;
    the five settled-row mean errors (constants.TRACKING_ERROR_NAMES) and `settled_rows`. A figure over nothing is nan."""
    vec = np.asarray(vec, np.float64)
    nan = float("nan")
    div = lambda a, b: float(a) / float(b) if b > 0 else nan
    envs, fell, rows, settled = (float(vec[S[k]]) for k in ("ENVS", "FELL_ENVS", "ROWS", "SETTLED"))
    out = dict(envs=int(envs), survival=div(envs - fell, envs), falls_per_s=div(vec[S["FALLS"]], rows * ctrl_dt),
               first_fall_s_mean=div(vec[S["FIRST_FALL_SUM"]], fell) * ctrl_dt, first_fall_s_min=float(vec[S["FIRST_FALL_MIN"]]) * ctrl_dt if fell > 0 else nan,
               timeouts=int(vec[S["TIMEOUTS"]]))
    for k, name in enumerate(constants.TRACKING_ERROR_NAMES):
        out[name] = div(vec[S["ERR_SUM"] + k], settled)
    out["settled_rows"] = int(settled)
    return out


def robustness_sweep(task, perturbations=None, commands=None, repeats: int = 8, seconds=None, settle_seconds=None, seed_offset: int = 7919):
    """The sweep behind HumanoidWalkingTask.robustness_sweep (see there): returns (entries, record) - one entry per case (perturbation x
    command, the commands of a perturbation in the order given), and the RobustnessRecord of what the run left behind. The default
    perturbations (default_perturbations) are settings of this build, not measured thresholds. Every call builds a context of its own and
    closes it again (host/sweep.py sweep_rollout)."""
    cfg, dev = task.config, task.device
    perts = default_perturbations() if perturbations is None else list(perturbations)
    commands = default_robustness_commands(task.kcfg) if commands is None else list(commands)
    if not perts or not commands or repeats < 1:
        raise ValueError("robustness_sweep needs at least one perturbation, one command and one repeat")
    if any(not isinstance(p, Perturbation) for p in perts):
        raise ValueError("robustness_sweep: a perturbation is a host/robustness.Perturbation")
    records = np.stack([p.record() for p in perts])                       # every refusal of the kernel, on the host, by field
    table = command_table(commands, "robustness_sweep: command {i}")
    cases = [(i, j) for i in range(len(perts)) for j in range(len(commands))]
    ncases = len(cases)
    n, group, (cmd_env, pert_env) = case_envs(task, ncases, repeats, f"robustness_sweep: {ncases} cases, kbj_robustness", table[[j for _, j in cases]],
                                              records[[i for i, _ in cases]])          # env e runs case e % ncases
    dt = cfg.ctrl_dt
    T = max(1, steps_of(cfg.render_length_seconds if seconds is None else seconds, dt))
    steps = settle_steps(cfg.tracking_settle_seconds if settle_seconds is None else settle_seconds, dt)
    status0 = torch.zeros(n, dtype=torch.int32, device=dev)
    keep = []

    def perturb(s):         # row 0: every env; behind a step: the envs whose episode has just started (their reset redrew the row)
        fresh = s.fresh()
        keep[:] = [None if fresh is None else fresh.to(torch.float32)]          # alive until the call has run (stream-ordered)
        s.ctx.env_perturb(keep[0], pert_env, status0 if fresh is None else None)

    with held_command_rollout(task, n, T, ScriptedCommand(cmd_env), seed_offset, after_resets=[perturb]) as (ctx, tr):
        err = torch.empty(T, n, L.TERR["SIZE"], device=dev)
        TrackingStats.fresh(ctx, tr.c, n, dev, steps, err=err)
        rec = torch.empty(n, R["SIZE"], dtype=torch.float64, device=dev)
        stats = torch.empty(ncases, S["SIZE"], dtype=torch.float64, device=dev)
        ctx.robustness(tr.c, err, rec, group, ncases, stats)
        ctx.synchronize()
        st = stats.cpu().numpy()
        ep = ctx.env_get_state()[0]
    if not bool((status0 == 1).all()):
        raise B.KbjError("robustness_sweep: kbj_env_perturb refused a record that Perturbation.record() had accepted")
    settings = dict(seconds=T * dt, settle=steps * dt, repeats=repeats)
    entries = [dict(perturbation=perts[i].name, changed=perts[i].changed(), command=tuple(float(x) for x in table[j]),
                    mode=constants.COMMAND_MODE_NAMES[command_mode(table[j])], in_training_range=in_training_range(perts[i], task.kcfg),
                    **settings, **case_summary(st[c], dt)) for c, (i, j) in enumerate(cases)]
    return entries, RobustnessRecord(tr.aux, err, rec, stats, group, pert_env, ep)


def format_robustness_table(entries) -> str:
    """robustness_sweep's result as a text table: under a line that echoes the settings one line per case - the perturbation by name (a `*`
    behind it where it lies outside the ranges the randomisers draw from), the command by its non-zero components, then the envs, the
    survival, the falls per second, the mean and earliest time of the first fall, the time-outs, the five settled-row mean errors and the
    settled rows ("-" over nothing)."""
    names = constants.TRACKING_ERROR_NAMES
    cols = ("survival", "falls_per_s", "first_fall_s_mean", "first_fall_s_min") + names
    heads = ("survival", "falls/s", "fall_s", "fall_s_min", "lin_err", "yaw_err", "tilt_err", "height_err", "arm_err")
    lines = []
    if entries:
        x = entries[0]
        lines.append(f"{x['seconds']:g} s per env, errors over the rows whose command has been held for {x['settle']:g} s, {x['repeats']} repeats; the perturbations are "
                     f"settings of this build, not measured thresholds; * = outside the ranges the training randomisers draw from")
    plabels = [x["perturbation"] + ("" if x["in_training_range"] else " *") for x in entries]
    clabels = [command_label(x["command"]) for x in entries]
    wp, wc = max([len("perturbation")] + [len(s) for s in plabels]), max([len("command")] + [len(s) for s in clabels])
    lines.append(f"{'perturbation':{wp}s}  {'command':{wc}s}  {'envs':>4s}" + "".join(f"  {h:>10s}" for h in heads[:4]) + f"  {'timeouts':>8s}"
                 + "".join(f"  {h:>10s}" for h in heads[4:]) + f"  {'settled':>8s}")
    for ps, cs, x in zip(plabels, clabels, entries):
        lines.append(f"{ps:{wp}s}  {cs:{wc}s}  {x['envs']:4d}" + "".join(table_cell(x[c]) for c in cols[:4]) + f"  {x['timeouts']:8d}"
                     + "".join(table_cell(x[c]) for c in cols[4:]) + f"  {x['settled_rows']:8d}")
    return "\n".join(lines)
