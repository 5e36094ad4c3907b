"""User-written Reset / Command / Observation / Termination terms in the reference's protocols (train.py:635, 682, 706, 724, 768, 817, 833),
and the step-wise rollout that runs them between the env step and the carry reset. Training (HumanoidWalkingTask.rollout) and
HumanoidWalkingTask.validate run the same loop, `UserTerms.run_steps`; each passes the hooks it wants, in the order it wants them."""
from __future__ import annotations

import torch

from ..spec import layout as L
from . import binding as B
from .traj_view import ResetData, StepView, combine_terminations

_DONE_BYTES = 4 * L.AUX["DONE"]       # the DONE column inside an aux row, as kbj_carry_reset takes it (base pointer + row stride)


class Step:
    """Observation row `row` of `tr` as a hook sees it: the state after control step `row - 1` (row 0: after the reset of all envs)."""

    def __init__(self, ctx, tr, row: int, step_index: int, model, qstate=None, term_rows=None):
        self.ctx, self.tr, self.row, self.step_index, self.model, self.qstate = ctx, tr, row, step_index, model, qstate
        self.term_rows = term_rows          # [N, ld_critic] terminal critic rows of the step that wrote this row (kbj_env_step_terminal), or None
        self.rows = (tr.actor_obs[row], tr.critic_obs[row], tr.aux[row])
        self.aux_prev = tr.aux[row - 1] if row else tr.aux[0]
        self._view = None

    def view(self) -> StepView:
        """The StepView of this row. It computes joint_position and its like eagerly, so a hook that rewrites the env state of the row calls
        `rewritten()` and the next hook gets a fresh one. (The command and the user columns, which the other hooks write, feed none of them.)"""
        if self._view is None:
            self._view = StepView(self.aux_prev, *self.rows, self.model, self.qstate)
        return self._view

    def rewritten(self):
        self._view = None

    def fresh(self):
        """[N] bool: the envs whose episode starts at this row; None on row 0, where every env's does."""
        return self.aux_prev[:, L.AUX["DONE"]] != 0 if self.row else None


class UserTerms:
    """The user's terms of one task, what they have produced (`obs_buffers`), and whether row 0 of a fresh task has been served (`started`)."""

    def __init__(self, terminations=None, observations=None, command=None, resets=None):
        self.terminations = dict(terminations or {})
        # an observation term may be given as (term, into) with into in {"actor", "critic", "both"}: its output is then ALSO written into the
        # networks' input rows, behind the reference's columns (config.extra_actor_obs / extra_critic_obs floats, in dictionary order)
        self.observations, self.obs_into = {}, {}
        for name, term in (observations or {}).items():
            into = None
            if isinstance(term, tuple):
                term, into = term
            into = into if into is not None else getattr(term, "into", None)
            if into not in (None, "actor", "critic", "both"):
                raise ValueError(f"observation {name!r}: into must be 'actor', 'critic', 'both' or None, not {into!r}")
            self.observations[name], self.obs_into[name] = term, into
        self.command_term = command
        self.resets = list(resets or [])
        self.obs_buffers: dict = {}           # {name: [T + 1, N, d]} of the training rollout
        self.started = False                  # row 0 of the first rollout has had its resets, command and observations (a resumed run's has)
        self.reset_keep = None                # the Reset terms' last result: alive until kbj_env_set_qstate has run (stream-ordered)
        self.seed = self.rank = self.device = self.model = self.nobs = None      # bind()

    def bind(self, seed: int, rank: int, device, model, nobs_actor: int, nobs_critic: int):
        """What the terms' calls need of the task, once it has a device: the generators' seed, the model, the networks' row widths."""
        self.seed, self.rank, self.device, self.model = seed, rank, device, model
        self.nobs = {"actor": nobs_actor, "critic": nobs_critic}

    def __bool__(self):
        return bool(self.terminations or self.observations or self.command_term is not None or self.resets)

    def _generator(self, a: int, b: int, step_index: int) -> torch.Generator:
        g = torch.Generator(device=self.device)
        g.manual_seed((self.seed * a + step_index * b + self.rank) & 0x7FFFFFFFFFFFFFFF)
        return g

    # ---- the hooks: each takes a Step, and does nothing without terms of its kind ----
    def apply_terminations(self, s: Step):
        """The user's Termination terms (train.py:817), OR-ed into the kernel's own: the env is reset (kbj_env_reset_where), GAE is cut there."""
        if not self.terminations:
            return
        done = s.aux_prev[:, L.AUX["DONE"]]
        user = combine_terminations(self.terminations, s.view())
        fire = (user != 0) & (done == 0)                # the kernel's own terminations already reset their envs
        if s.term_rows is not None:                     # this env's critic row as the step left it IS its terminal row: keep it before the reset rewrites it
            s.term_rows.copy_(torch.where(fire[:, None], s.rows[1], s.term_rows))
        s.ctx.env_reset_where(fire.to(torch.float32), *s.rows)
        s.aux_prev[:, L.AUX["DONE"]] = torch.where(fire, user, done)
        s.rewritten()

    def apply_resets(self, s: Step):
        """The user's Reset terms (train.py:833-844): evaluated on every env's (qpos, qvel), kept for the envs whose episode starts at this row,
        written back - with the rows of the next observation - by kbj_env_set_qstate."""
        if not self.resets:
            return
        n = s.rows[2].shape[0]
        qpos, qvel = torch.empty(n, L.NQ, device=self.device), torch.empty(n, L.NV, device=self.device)
        s.ctx.env_get_qstate(qpos, qvel)
        g = self._generator(2246822519, 3266489917, s.step_index)
        data = ResetData(qpos, qvel)
        for term in self.resets:
            data = term(data, 1.0, g)
            # a Reset term returns the data it was given with fields replaced (train.py:833-844): same shapes, finite numbers. Checked here, by name,
            # on the host (this is the step-wise path of user terms, not the fused rollout): the kernel would carry a NaN into the observation
            # rows without a word, and a broadcastable wrong shape would only surface as a reshape error further down.
            for field, width in (("qpos", L.NQ), ("qvel", L.NV)):
                v = getattr(data, field, None)
                if not torch.is_tensor(v) or tuple(v.shape) != (n, width):
                    raise B.KbjError(f"Reset term {type(term).__name__} returned {field} of shape {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}, "
                                     f"expected ({n}, {width})")
                if not bool(torch.isfinite(v).all()):
                    raise B.KbjError(f"Reset term {type(term).__name__} returned non-finite values in {field}")
        self.reset_keep = (data.qpos.to(torch.float32).contiguous(), data.qvel.to(torch.float32).contiguous())
        fresh = s.fresh()
        s.ctx.env_set_qstate(None if fresh is None else fresh.to(torch.float32), *self.reset_keep, *s.rows)
        s.rewritten()

    def apply_command(self, s: Step):
        """The user's Command term (train.py:724, 768): `initial_command` for the envs whose episode starts at this row, `__call__(prev_command,
        ...)` for the others, written by kbj_env_set_command. On row 0 every env starts one; elsewhere both are evaluated and selected on the
        device - asking `fresh.all()` would drain the queue once per control step."""
        term = self.command_term
        if term is None:
            return
        aux, view = s.rows[2], s.view()
        n = aux.shape[0]
        g = self._generator(2654435761, 40503, s.step_index)
        prev = aux[:, L.AUX["CMD"]:L.AUX["CMD"] + L.NCMD].clone()
        new = term.initial_command(view, 1.0, g).reshape(n, L.NCMD).to(torch.float32)
        fresh = s.fresh()
        if fresh is not None:
            new = torch.where(fresh[:, None], new, term(prev, view, 1.0, g).reshape(n, L.NCMD).to(torch.float32))
        s.ctx.env_set_command(None, new.contiguous(), *s.rows)

    def observe_rows(self, s: Step) -> dict:
        """Evaluate the user's Observation terms (train.py:635, 682, 706) and write those routed into the networks behind the reference's
        columns of this row (actor: from column 65, critic: from 475, dictionary order). Returns {name: [N, d]}."""
        view = s.view()
        ref = {"actor": L.NOBS_ACTOR, "critic": L.NOBS_CRITIC}
        off, rows, lim = dict(ref), {"actor": s.rows[0], "critic": s.rows[1]}, self.nobs
        out = {}
        for name, term in self.observations.items():
            v = term.observe(view, 1.0, None) if hasattr(term, "observe") else term(view)
            v = v.reshape(view.N, -1).to(torch.float32)
            out[name] = v
            into = self.obs_into.get(name)
            for net in (("actor", "critic") if into == "both" else (into,) if into else ()):
                if off[net] + v.shape[1] > lim[net]:
                    raise B.KbjError(f"observation {name!r} ({v.shape[1]} floats) does not fit the {net} row: config.extra_{net}_obs reserves "
                                     f"{lim[net] - ref[net]} floats")
                rows[net][:, off[net]:off[net] + v.shape[1]] = v
                off[net] += v.shape[1]
        for net in ("actor", "critic"):
            if any(i in (net, "both") for i in self.obs_into.values()) and off[net] != lim[net]:
                raise B.KbjError(f"the observation terms routed into the {net} fill {off[net] - ref[net]} "
                                 f"floats, config.extra_{net}_obs says {lim[net] - ref[net]}")
        return out

    def observe(self, s: Step):
        """observe_rows, and every term's answer kept as row `row` of `obs_buffers[name]` for the Python reward / termination terms."""
        if not self.observations:
            return
        for name, v in self.observe_rows(s).items():
            if name not in self.obs_buffers:
                self.obs_buffers[name] = torch.zeros(s.tr.aux.shape[0], v.shape[0], v.shape[1], device=self.device)
            self.obs_buffers[name][s.row].copy_(v)

    # ---- the loop ----
    def run_hooks(self, ctx, tr, row: int, step_index: int, hooks, qstate=None, term_rows=None):
        s = Step(ctx, tr, row, step_index, self.model, qstate, term_rows)
        for hook in hooks:
            hook(s)

    def run_steps(self, ctx, tr, carry, params, T: int, seed: int, first_step: int, argmax: bool, first_index: int, hooks, terminal: bool = False):
        """kbj_rollout's T control steps as separate ABI calls - policy step, env step, `hooks` in list order on the row the env step wrote,
        carry reset: the same calls kbj_rollout fuses, bit-identical when no hook changes anything. The policy draws step `first_step + t` of
        `seed`; the hooks of row t + 1 get the step index `first_index + t + 1`. terminal (a context with kbj_config.gae_terminal_value): as
        kbj_rollout does then, the env step is kbj_env_step_terminal into tr.term_rows, and kbj_critic_terminal_value writes tr.value_term[t]
        in front of the carry reset - behind the hooks, so that a user Termination term's +1 and its terminal row count."""
        for t in range(T):
            qs = tr.qstate[t] if tr.qstate is not None else None
            done = tr.aux[t].data_ptr() + _DONE_BYTES
            ctx.policy_step(params, tr.actor_obs[t], tr.critic_obs[t], carry.c, seed, first_step + t, argmax, tr.action[t], tr.logp[t], tr.value[t])
            if terminal:
                ctx.env_step_terminal(tr.action[t], tr.aux[t], tr.actor_obs[t + 1], tr.critic_obs[t + 1], tr.aux[t + 1], tr.term_rows)
            else:
                ctx.env_step(tr.action[t], tr.aux[t], tr.actor_obs[t + 1], tr.critic_obs[t + 1], tr.aux[t + 1], qs)
            self.run_hooks(ctx, tr, t + 1, first_index + t + 1, hooks, qs, tr.term_rows if terminal else None)
            if terminal:
                ctx.critic_terminal_value(params, tr.term_rows, carry.c, done, L.AUX["SIZE"], tr.value_term[t])
            ctx.carry_reset(carry.c, done, L.AUX["SIZE"])
