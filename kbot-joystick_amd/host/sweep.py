"""What the evaluation sweeps (host/tracking.py tracking_sweep, host/push.py push_sweep, host/gait.py gait_sweep, host/step.py step_sweep,
host/actuator.py actuator_sweep, host/frequency.py frequency_sweep) share: a context of their own for n envs and T rows,
one rollout with the task's policy acting with the distribution's mode, the user terms the sweep scripts."""
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


def case_of_env(n: int, ncases: int, device) -> torch.Tensor:
    """The group tensor of a sweep's statistics call: env e runs case e % ncases."""
    return (torch.arange(n, device=device) % ncases).to(torch.int32)


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


def held_command_rollout(task, n: int, T: int, command, seed_offset: int, record_state: bool = False):
    """sweep_rollout under the Command term `command` alone (tracking, gait, step, actuator and frequency sweeps): command_mode = 1, so that the kernel's own
    reset writes the context's fixed command and the term's answer then replaces it, and validate()'s hook order - on row 0 the resets, the
    command, then the observation terms that feed a network; behind every step the resets, those observation terms, then the command."""
    terms = sweep_terms(task, command=command)
    feeds = [terms.observe_rows] if any(task.extra_obs) else []

    def configure(vcfg):
        vcfg.command_mode = 1

    return sweep_rollout(task, n, T, configure, terms, [terms.apply_resets, terms.apply_command] + feeds,
                         [terms.apply_resets] + feeds + [terms.apply_command], seed_offset, record_state)
