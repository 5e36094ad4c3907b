"""User-written Reset / Command / Observation / Termination terms in the reference's protocols (train.py:635, 682, 706, 724, 768, 817, 833),
Event terms in this build's own protocol (apply_events), and the step-wise rollout that runs them between the env step and the carry reset. Training (HumanoidWalkingTask.rollout) and
HumanoidWalkingTask.validate run the same loop, `UserTerms.run_steps`; each passes the hooks it wants, in the order it wants them."""
from __future__ import annotations

import weakref

import torch

from ..spec import layout as L
from . import binding as B
from .traj_view import PushRequest, ResetData, StepView, combine_terminations

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
            self._view.row = self.row
        return self._view

    def rewritten(self):
        self._view = None

    def fresh(self):
        """[N] bool: the envs whose episode starts at this row; None on row 0, where every env's does."""
        return self.aux_prev[:, L.AUX["DONE"]] != 0 if self.row else None


def check_push_request(name: str, req, n: int) -> PushRequest:
    """An Event term's PushRequest for n envs, checked by field - shapes, then (one read-back) the values of the masked envs: finite, steps and
    next whole numbers in [0, PUSH_NEVER] - and returned with float32 fields. Raises KbjError naming the term and the field."""
    if not isinstance(req, PushRequest):
        raise B.KbjError(f"Event term {name!r} returned {type(req).__name__} as its push, expected None or a PushRequest")
    shapes = dict(mask=(n,), wrench=(n, 6), steps=(n,), next=(n,))
    for field, shape in shapes.items():
        v = getattr(req, field)
        if field == "next" and v is None:
            continue
        if not torch.is_tensor(v) or tuple(v.shape) != shape:
            raise B.KbjError(f"Event term {name!r} returned {field} of shape {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}, expected {shape}")
    if req.mask.dtype != torch.bool:
        raise B.KbjError(f"Event term {name!r} returned a mask of dtype {req.mask.dtype}, expected torch.bool")
    m = req.mask
    wrench, steps = req.wrench.to(torch.float32), req.steps.to(torch.float32)
    nxt = None if req.next is None else req.next.to(torch.float32)
    counts = lambda v: torch.isfinite(v) & (v == torch.floor(v)) & (v >= 0) & (v <= L.PUSH_NEVER)
    bad = [(m[:, None] & ~torch.isfinite(wrench)).any(), (m & ~counts(steps)).any()] + ([(m & ~counts(nxt)).any()] if nxt is not None else [])
    bad = torch.stack(bad).tolist()
    if bad[0]:
        raise B.KbjError(f"Event term {name!r} returned non-finite values in wrench")
    for field, b in zip(("steps", "next"), bad[1:]):
        if b:
            raise B.KbjError(f"Event term {name!r} returned {field} that are not whole numbers in [0, {int(L.PUSH_NEVER)}] (control steps)")
    return PushRequest(m, wrench, steps, nxt)


class UserTerms:
    """The user's terms of one task, what they have produced (`obs_buffers`), and whether row 0 of a fresh task has been served (`started`)."""

    def __init__(self, terminations=None, observations=None, command=None, resets=None, events=None):
        self.terminations = dict(terminations or {})
        self.events = dict(events or {})
        # what each Event term carries from row to row, PER CONTEXT ({ctx: {name: [N, ...] tensor or None}}): the training rollout and a
        # validation run drive different env sets through the same terms, and neither may see the other's state
        self.event_states = weakref.WeakKeyDictionary()
        self.push_keep = None                 # the last kbj_env_set_push arguments: alive until the call has run (stream-ordered)
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
        return bool(self.terminations or self.observations or self.command_term is not None or self.resets or self.events)

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

    def event_state_of(self, ctx) -> dict:
        """{name: event state} of the Event terms for the env set of `ctx` (created empty; dropped with the context)."""
        if ctx not in self.event_states:
            self.event_states[ctx] = {}
        return self.event_states[ctx]

    def apply_events(self, s: Step):
        """The user's Event terms, in dictionary order. The reference lists its events in get_events (train.py:1134-1144), but ksim's Event
        class is un-vendored: THIS PROTOCOL IS THIS BUILD'S OWN, shaped after the Command protocol beside it. A term is called once per row:
          `term.initial_event_state(state, curriculum_level, rng) -> [N, ...] tensor` (optional): the state the term carries, for the envs whose
              episode starts at this row (all of them on row 0); without it the term carries what its first call returns, or None;
          `term(state, event_state, curriculum_level, rng) -> (push, event_state)`: `push` is None or a traj_view.PushRequest.
        `state` is the row's StepView (state.row: the trajectory row), `rng` a torch.Generator seeded from (seed, step index). Later terms win
        on the envs they mask. The merged request goes to kbj_env_set_push: the wrench acts from the NEXT control step on, for `steps` steps;
        no observation changes. An in-step reset clears a running push and re-arms the built-in event: a term that scripts pushes writes
        `next` again on fresh envs. Checked here, on the host (this is the step-wise path, as in apply_resets): shapes, finite values, and
        whole-numbered steps / next in [0, PUSH_NEVER] - on the masked envs, the only ones read. The event state belongs to the context the
        row was stepped by (`event_state_of`): a validation run starts its own and leaves the training run's alone."""
        if not self.events:
            return
        state = self.event_state_of(s.ctx)
        view, fresh = s.view(), s.fresh()
        n = s.rows[2].shape[0]
        g = self._generator(1597334677, 2869860233, s.step_index)
        f32 = dict(dtype=torch.float32, device=self.device)
        mask, wrench, steps, nxt = torch.zeros(n, dtype=torch.bool, device=self.device), torch.zeros(n, 6, **f32), torch.zeros(n, **f32), torch.zeros(n, **f32)
        has_next = torch.zeros(n, dtype=torch.bool, device=self.device)
        asked, with_next = 0, 0
        for name, term in self.events.items():
            st = state.get(name)
            if hasattr(term, "initial_event_state"):      # both are evaluated and selected on the device, as apply_command does
                init = term.initial_event_state(view, 1.0, g)
                st = init if fresh is None or st is None else torch.where(fresh.reshape((n,) + (1,) * (init.dim() - 1)), init, st)
            out = term(view, st, 1.0, g)
            if not (isinstance(out, tuple) and len(out) == 2):
                raise B.KbjError(f"Event term {name!r} must return (push, event_state), got {type(out).__name__}")
            req, state[name] = out
            if req is None:
                continue
            req = check_push_request(name, req, n)
            m = req.mask
            mask = mask | m
            wrench, steps = torch.where(m[:, None], req.wrench, wrench), torch.where(m, req.steps, steps)
            asked += 1
            if req.next is not None:
                nxt, has_next = torch.where(m, req.next, nxt), has_next | m
                with_next += 1
            else:
                has_next = has_next & ~m
        if not asked:
            return
        self.push_keep = (mask.to(torch.float32), wrench.contiguous(), steps.contiguous(), nxt.contiguous(), (mask & has_next).to(torch.float32), (mask & ~has_next).to(torch.float32))
        m_all, w, st_, nx, m_next, m_plain = self.push_keep
        if with_next == 0:
            s.ctx.env_set_push(m_all, w, st_, None)
        elif with_next == asked:          # every request names `next`: has_next covers the mask
            s.ctx.env_set_push(m_all, w, st_, nx)
        else:                             # which envs end up with a `next` is only known on the device: one call for each kind
            s.ctx.env_set_push(m_plain, w, st_, None)
            s.ctx.env_set_push(m_next, w, st_, nx)

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
