"""What the evaluation sweeps (host/tracking.py tracking_sweep, host/push.py push_sweep, host/gait.py gait_sweep, host/step.py step_sweep,
host/actuator.py actuator_sweep, host/frequency.py frequency_sweep) share: a context of their own for n envs and T rows,
one rollout with the task's policy acting with the distribution's mode, the user terms the sweep scripts - and, for the sweeps over held
commands and for those over cases, the envs, tables and entries around their own measurement."""
from __future__ import annotations

import contextlib
import dataclasses

import numpy as np
import torch

from ..spec import constants, layout as L
from . import binding as B
from .buffers import CarryBuffers, TrajBuffers
from .user_terms import UserTerms


def steps_of(seconds: float, ctrl_dt: float) -> int:
    return int(round(seconds / ctrl_dt))


def command_table(commands, what: str = "command {i}") -> np.ndarray:
    """Commands of up to 16 components as a [len, 16] float32 table, the missing components zero. `what` names command i in the error."""
    table = np.zeros((len(commands), L.NCMD), np.float32)
    for i, c in enumerate(commands):
        c = np.asarray(c, np.float32).reshape(-1)
        if c.size > L.NCMD:
            raise ValueError(f"{what.format(i=i)} has {c.size} components, a command has {L.NCMD}")
        table[i, :c.size] = c
    return table


def command_label(cmd) -> str:
    """A command as a table label: its non-zero components by name."""
    parts = [f"{constants.COMMAND_NAMES[k]}={v:+.2f}" for k, v in enumerate(cmd) if v != 0]
    return " ".join(parts) if parts else "(zero)"


def table_cell(v) -> str:
    """A figure as a 10-wide table cell, "-" over nothing (nan)."""
    return f"  {'-':>10s}" if v != v else f"  {v:10.3f}"


def per_env_table(table, repeats: int, device) -> torch.Tensor:
    """A per-case table [cases, ...] as the per-env table on the device: env e takes row e % cases."""
    return torch.from_numpy(np.tile(table, (repeats, 1))).to(device)


def case_envs(task, ncases: int, repeats: int, too_many: str, *tables):
    """The envs of a case sweep (push, step, frequency): (n, group, per-env tables) - ncases * repeats envs, the group tensor of the
    statistics call and every per-case table of `tables` per env on the device. The group reduce takes at most 256 cases: more are
    refused as "<too_many> groups at most 256", before the device is touched."""
    if ncases > 256:
        raise ValueError(f"{too_many} groups at most 256")
    n, dev = ncases * repeats, task.device
    return n, (torch.arange(n, device=dev) % ncases).to(torch.int32), [per_env_table(t, repeats, dev) for t in tables]


def failures_per_s(done, envs, seconds: float) -> float:
    """Falls (DONE < 0) of the envs `envs` in done [T, N], per second of the `seconds` they ran together."""
    return float(sum((done[:, j] < 0).sum() for j in envs)) / seconds


def sweep_terms(task, command=None, events=None) -> UserTerms:
    """The task's observation terms (those that feed a network) and reset terms, beside the sweep's own Command or Event terms."""
    return UserTerms(None, {name: (term, task.terms.obs_into[name]) for name, term in task.terms.observations.items() if task.terms.obs_into[name]},
                     command, task.terms.resets, events)


@contextlib.contextmanager
def sweep_rollout(task, n: int, T: int, configure, terms: UserTerms, first_hooks, step_hooks, seed_offset: int, record_state: bool = False):
    """Run T control steps of n envs on a context built for the sweep and hand back (ctx, tr) - the context and its TrajBuffers - for the
    sweep's statistics; the context is closed when the block ends. The kbj_config is the task's for n envs and T rows with GAE off (no tail
    pass, no terminal rows), then `configure(vcfg)`. `terms` are bound here; `first_hooks` run on row 0 behind the reset, `step_hooks` behind
    every step (UserTerms.run_hooks / run_steps: the caller's order is kept). Seeds and draw indices start at `seed_offset`.
    record_state: the TrajBuffers also keep the state record of every step (tr.qstate; the actuator sweep reads joint positions and speeds there).
    Every call builds its context and closes it again (validate() caches its own; a sweep is asked for now and then, and its env count
    follows its cases)."""
    cfg, dev = task.config, task.device
    vcfg = dataclasses.replace(cfg, batch_size=n).to_kbj(n)
    vcfg.rollout_len = T
    vcfg.gae_bootstrap_truncation = vcfg.gae_tail_value = vcfg.gae_terminal_value = 0
    configure(vcfg)
    terms.bind(cfg.seed, task.rank, dev, task.model_blob, task.nobs_actor, task.nobs_critic)
    ctx = B.Context(task.model_blob, vcfg, dev.index or 0, torch.cuda.current_stream().cuda_stream)
    try:
        carry = CarryBuffers(n, task.H, task.kcfg.depth, dev, mirror=task.mirror)
        tr = TrajBuffers(T, n, task.H, task.kcfg.depth, dev, mirror=task.mirror, ld_actor=task.ld_actor, ld_critic=task.ld_critic, record_state=record_state)
        seed = cfg.seed + seed_offset
        ctx.env_reset_all(seed, tr.actor_obs[0], tr.critic_obs[0], tr.aux[0])
        terms.run_hooks(ctx, tr, 0, seed_offset, first_hooks)
        terms.run_steps(ctx, tr, carry, task.params, T, seed=seed, first_step=0, argmax=True, first_index=seed_offset, hooks=step_hooks)
        yield ctx, tr
    finally:
        ctx.close()


def held_command_rollout(task, n: int, T: int, command, seed_offset: int, record_state: bool = False, after_resets=()):
    """sweep_rollout under the Command term `command` alone (tracking, gait, step, actuator, frequency and robustness sweeps): command_mode = 1, so that the kernel's own
    reset writes the context's fixed command and the term's answer then replaces it, and validate()'s hook order - on row 0 the resets, the
    command, then the observation terms that feed a network; behind every step the resets, those observation terms, then the command.
    `after_resets`: further hooks of the sweep's own, run on every row behind the resets and in front of everything else (the robustness
    sweep writes its model rows there)."""
    terms = sweep_terms(task, command=command)
    feeds = [terms.observe_rows] if any(task.extra_obs) else []
    own = list(after_resets)

    def configure(vcfg):
        vcfg.command_mode = 1

    return sweep_rollout(task, n, T, configure, terms, [terms.apply_resets] + own + [terms.apply_command] + feeds,
                         [terms.apply_resets] + own + feeds + [terms.apply_command], seed_offset, record_state)


# ---- the command sweeps (tracking, gait, actuator): one held command per env ----
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


def command_mode(cmd) -> int:
    """The KBJ_CMODE of one command (include/kbj.h kbj_tracking_stats): which of cmd[0:3] are non-zero, and whether any of cmd[3:16] is."""
    c = np.asarray(cmd, np.float32)
    nz, pose = c[:3] != 0, bool((c[3:] != 0).any())
    if not nz.any():
        return L.CMODE["STAND_BEND"] if pose else L.CMODE["STAND"]
    if pose or nz.sum() != 1:
        return L.CMODE["OMNI"]
    return int(np.argmax(nz))


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


@contextlib.contextmanager
def command_sweep(task, name: str, commands, repeats: int, seconds, seed_offset: int, **rollout):
    """The rollout of the sweep `name` (tracking_sweep, gait_sweep, actuator_sweep): len(commands) * repeats envs (default commands:
    default_command_grid; env e follows command e % len(commands)), `seconds` (default render_length_seconds) under a ScriptedCommand term
    that hands every env its own command again after an in-episode reset. The block gets (ctx, tr, n, T, entries) and queues its
    statistics call on `ctx`, which is closed when the block ends. `entries(measured)` then builds the table: one dict per command -
    `command`, `mode`, `measured(envs)`, the sweep's own figures over the command's envs, and `failures_per_s`. `rollout`: further
    arguments of held_command_rollout (record_state)."""
    cfg = task.config
    commands = default_command_grid(task.kcfg) if commands is None else commands
    if len(commands) == 0 or repeats < 1:
        raise ValueError(f"{name} needs at least one command and one repeat")
    table = command_table(commands)
    ncmd, n = len(commands), len(commands) * repeats
    T = max(1, int(round((cfg.render_length_seconds if seconds is None else seconds) / cfg.ctrl_dt)))

    def entries(measured) -> list:
        out, done = [], tr.done.cpu().numpy()
        for i in range(ncmd):
            envs = list(range(i, n, ncmd))
            entry = dict(command=tuple(float(x) for x in table[i]), mode=constants.COMMAND_MODE_NAMES[command_mode(table[i])])
            entry.update(measured(envs))
            entry["failures_per_s"] = failures_per_s(done, envs, repeats * T * cfg.ctrl_dt)
            out.append(entry)
        return out
    with held_command_rollout(task, n, T, ScriptedCommand(per_env_table(table, repeats, task.device)), seed_offset, **rollout) as (ctx, tr):
        yield ctx, tr, n, T, entries


def format_command_table(entries, columns, last=None) -> str:
    """A command sweep's entries as a text table: one line per command (its non-zero components by name) and its mode, then a 10-wide cell
    per (title, key) of `columns` ("-" where there was nothing to average). `last`: the (title, key) of a closing column printed as it is."""
    labels = [command_label(x["command"]) for x in entries]
    w = max([len("command")] + [len(s) for s in labels])
    lines = [f"{'command':{w}s}  {'mode':10s}" + "".join(f"  {title:>10s}" for title, _ in columns) + (f"  {last[0]}" if last else "")]
    for s, x in zip(labels, entries):
        lines.append(f"{s:{w}s}  {x['mode']:10s}" + "".join(table_cell(x[key]) for _, key in columns) + (f"  {x[last[1]]}" if last else ""))
    return "\n".join(lines)
