"""What the evaluation sweeps (host/tracking.py tracking_sweep, host/push.py push_sweep, host/gait.py gait_sweep, host/step.py step_sweep) share: a context of their own for n envs and T rows,
one rollout with the task's policy acting with the distribution's mode, the user terms the sweep scripts."""
from __future__ import annotations

import contextlib
import dataclasses

import torch

from . import binding as B
from .buffers import CarryBuffers, TrajBuffers
from .user_terms import UserTerms


def sweep_terms(task, command=None, events=None) -> UserTerms:
    """The task's observation terms (those that feed a network) and reset terms, beside the sweep's own Command or Event terms."""
    return UserTerms(None, {name: (term, task.terms.obs_into[name]) for name, term in task.terms.observations.items() if task.terms.obs_into[name]},
                     command, task.terms.resets, events)


@contextlib.contextmanager
def sweep_rollout(task, n: int, T: int, configure, terms: UserTerms, first_hooks, step_hooks, seed_offset: int):
    """Run T control steps of n envs on a context built for the sweep and hand back (ctx, tr) - the context and its TrajBuffers - for the
    sweep's statistics; the context is closed when the block ends. The kbj_config is the task's for n envs and T rows with GAE off (no tail
    pass, no terminal rows), then `configure(vcfg)`. `terms` are bound here; `first_hooks` run on row 0 behind the reset, `step_hooks` behind
    every step (UserTerms.run_hooks / run_steps: the caller's order is kept). Seeds and draw indices start at `seed_offset`.
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
        tr = TrajBuffers(T, n, task.H, task.kcfg.depth, dev, mirror=task.mirror, ld_actor=task.ld_actor, ld_critic=task.ld_critic)
        seed = cfg.seed + seed_offset
        ctx.env_reset_all(seed, tr.actor_obs[0], tr.critic_obs[0], tr.aux[0])
        terms.run_hooks(ctx, tr, 0, seed_offset, first_hooks)
        terms.run_steps(ctx, tr, carry, task.params, T, seed=seed, first_step=0, argmax=True, first_index=seed_offset, hooks=step_hooks)
        yield ctx, tr
    finally:
        ctx.close()
