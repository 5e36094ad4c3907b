"""Host-side mirror of the reference's task interface for the hot path.

The reference's boundary is ksim's Python Task API: `HumanoidWalkingTask(ksim.PPOTask[Config])`
(train.py:1058) driven by `HumanoidWalkingTask.launch(HumanoidWalkingTaskConfig(...))` (train.py:1759-1792).
This module keeps those names, argument meanings and error behaviour for the path that was rebuilt
(rollout + PPO update), and routes them to libkbj.so. What the reference delegates to ksim/xax outside the
hot path (viewer, TensorBoard, CLI parsing) is out of scope.
"""
from __future__ import annotations

import dataclasses
import os
import sys
import threading
import time
import warnings
from typing import NamedTuple, Optional

import numpy as np
import torch

from ..spec import compiler, constants, layout as L
from . import binding as B
from . import ckpt as ckpt_io
from . import dist as dist_util
from . import wiring
from .buffers import CarryBuffers, TrajBuffers
from .actuator import ActuatorStats, actuator_joint_table, actuator_sweep, format_actuator_joint_table, format_actuator_table, levels_of_config      # noqa: F401 (re-exported)
from .ckpt import ModelView
from .config import HumanoidWalkingTaskConfig, cosine_decay_lr, launch_config      # launch_config: re-exported with the rest
from .episode import EpisodeStats, episode_stats_scalars      # noqa: F401 (re-exported)
from .frequency import FrequencyRecord, SineCommand, format_frequency_table, frequency_sweep      # noqa: F401 (re-exported)
from .gait import GaitStats, format_gait_table, gait_sweep      # noqa: F401 (re-exported)
from .push import PushRecord, ScriptedPush, format_push_table, push_sweep      # noqa: F401 (re-exported)
from .robustness import Perturbation, RobustnessRecord, format_robustness_table, in_training_range, robustness_sweep      # noqa: F401 (re-exported)
from .step import StepRecord, SteppedCommand, format_step_table, step_sweep      # noqa: F401 (re-exported)
from .tracking import TrackingStats, format_tracking_table, settle_steps, tracking_sweep      # noqa: F401 (re-exported)
from .user_terms import UserTerms


_NO_PREFETCH = os.environ.get("KBJ_NO_PREFETCH", "0") not in ("0", "")     # A/B switch: kbj_ppo_prefetch is a pure scheduling hint


class _Validation(NamedTuple):
    """The cached context and buffers of validate() / view(), for its (num_envs, T)."""
    key: tuple
    ctx: B.Context
    carry: CarryBuffers
    traj: TrajBuffers


class HumanoidWalkingTask:
    """Rollout + PPO update of the K-Bot joystick task on one GPU of a data-parallel job.

    Environments are sharded over ranks (rank r owns global env ids [r*N, (r+1)*N)); the only exchange step is
    the gradient all-reduce before each optimizer step.
    """

    def __init__(self, config: HumanoidWalkingTaskConfig, device: Optional[torch.device] = None, rank: int = 0, world_size: int = 1,
                 extra_rewards: Optional[dict] = None, extra_terminations: Optional[dict] = None, extra_observations: Optional[dict] = None,
                 command=None, extra_resets: Optional[list] = None, extra_events: Optional[dict] = None):
        """extra_rewards: {name: term} of Python reward terms in ksim's Reward protocol (`scale`, `get_reward(trajectory)` or the stateful
        pair), evaluated on `TrajectoryView` after every rollout and added to the built-in stack's reward (host/traj_view.py).
        extra_terminations: {name: term}, `term(state, curriculum_level) -> [N] in {-1, 0, 1}` (train.py:817) on a `StepView` after every
        control step, OR-ed into the kernel's own terminations: the env is reset (kbj_env_reset_where), the model carries with it, GAE is
        cut there. extra_observations: {name: term}, `term.observe(state, curriculum_level, rng)` or a plain callable -> [N, d]
        (train.py:635, 682, 706), evaluated per control step and kept as [T + 1, N, d] tensors for the Python reward / termination terms
        (`TrajectoryView.extra_observations[name]`); the networks' input rows stay the reference's 65 / 475 floats.
        command: ONE term in the reference's Command protocol (train.py:724, 768) that replaces the built-in UnifiedCommand sampler:
        `command.initial_command(state, curriculum_level, rng) -> [N, 16]` for the envs that have just been reset and
        `command(prev_command, state, curriculum_level, rng) -> [N, 16]` for the running ones, evaluated on the device after every
        control step and written into the env state and the next observation rows by kbj_env_set_command (`rng` is a torch.Generator of
        the task's device, seeded from (seed, step index)). The library then runs with command_mode = 1 so its own switch draw stays off.
        extra_resets: a LIST of terms in the reference's Reset protocol (train.py:833-844: `term(data, curriculum_level, rng) -> data` with
        `data.qpos` / `data.qvel`), applied in list order - behind the built-in resets of train.py:1146-1153, as further entries of that list would
        be - to the envs that have just been re-initialised; the result is written back by kbj_env_set_qstate, which also rewrites their next
        observation rows (host/traj_view.ResetData; `rng` is a torch.Generator seeded from (seed, step index)).
        extra_events: {name: term} of Event terms - scripted disturbances beside the built-in ForcePushEvent of get_events() (train.py:1134-1144).
        ksim's Event class is un-vendored, so the protocol is this build's own (host/user_terms.py apply_events): optional
        `term.initial_event_state(state, curriculum_level, rng)`, and `term(state, event_state, curriculum_level, rng) -> (push, event_state)` with
        `push` None or a `traj_view.PushRequest(mask, wrench, steps[, next])`, evaluated after every control step behind the Reset terms and in
        front of the Command term; the wrench is written into the env state by kbj_env_set_push and acts from the next control step on. Needs
        the built-in event's switch on (`enable_pushes`; checked here): the step kernel reads the event state only then. Event state is kept per
        library context - validate() runs the terms on a state of its own, started afresh every time - and is not checkpointed: a resumed
        run starts it from `initial_event_state`.
        With any of these the rollout runs step by step from the host (policy step, env step, user terms, carry reset: the same calls
        kbj_rollout fuses, bit-identical when no user term fires) instead of as one kbj_rollout call."""
        self.extra_rewards = dict(extra_rewards or {})
        self.terms = UserTerms(extra_terminations, extra_observations, command, extra_resets, extra_events)     # host/user_terms.py
        self.extra_obs_buffers = self.terms.obs_buffers
        self._extra_carries: dict = {}
        self.extra_reward_means: dict = {}
        # state that comes into being later: update()'s permutation staging and exchange stream, validate()'s cache, the checkpoint writer
        self._perm_pinned = self._perm_dev = self._perm_event = None
        self._comm_stream = None
        self._adv_sums = None                  # the last global advantage sums: alive until kbj_set_advantage_sums' consumer has run
        self._warned_ascent = False
        self._valid: Optional[_Validation] = None
        self._save_thread = self._save_error = None
        self.loop_stats: Optional[dict] = None  # launch()'s account of its loop
        if not torch.cuda.is_available():
            raise B.KbjError("HumanoidWalkingTask needs a HIP device (no CPU fallback)")
        self.config = config
        self.rank, self.world_size = rank, world_size
        if config.run_mode not in ("train", "view"):
            raise ValueError(f"run_mode must be 'train' or 'view' (README.md:66-70), not {config.run_mode!r}")
        if config.use_lr_decay and config.adam_weight_decay == 0.0 and config.reproduce_reference_lr_sign:
            # every rank, at construction: a single warnings.warn is easy to lose in a multi-rank log
            print(f"[kbj rank {rank}] reproduce_reference_lr_sign: optax.chain(scale_by_adam, scale_by_schedule) as written in "
                  "train.py:1074-1075 has no sign flip - this run ASCENDS the loss", file=sys.stderr, flush=True)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.N, env_off = dist_util.env_shard(config.num_envs, rank, world_size)
        self.kcfg = config.to_kbj(self.N, env_id_offset=env_off)
        if command is not None:
            self.kcfg.command_mode = 1          # resets write fixed_command (zeros unless configured); the term overwrites it every step
        if self.terms.events and not self.kcfg.enable_pushes:
            raise ValueError("extra_events needs the push event's switch on (kbj_config.enable_pushes = 1): with it off the step kernel ignores the event "
                             "state kbj_env_set_push writes, and the library refuses the call")
        self.T, self.H, self.B = self.kcfg.rollout_len, self.kcfg.hidden_size, self.kcfg.batch_size
        self.model_blob = self.get_mujoco_model()
        torch.cuda.set_device(self.device)     # torch ops of this task and the library's launches must target the same GPU
        self.ctx = B.Context(self.model_blob, self.kcfg, self.device.index or 0, torch.cuda.current_stream().cuda_stream)
        self.P = self.ctx.param_count()
        self.params = self.get_model(config.seed)
        self.opt_m = torch.zeros_like(self.params)
        self.opt_v = torch.zeros_like(self.params)
        self.grad = torch.zeros_like(self.params)
        self.grad_acc = torch.zeros_like(self.params) if config.allreduce == "per_pass" else None
        self.metrics = torch.zeros(10, device=self.device)
        self.mirror = config.actor_mirror_loss_scale != 0.0 or config.critic_mirror_loss_scale != 0.0
        self.carry = self.get_initial_model_carry()
        self.nobs_actor, self.nobs_critic, self.ld_actor, self.ld_critic = L.obs_widths(self.kcfg)
        self.extra_obs = (int(self.kcfg.extra_obs_actor), int(self.kcfg.extra_obs_critic))
        if any(self.extra_obs) and not any(v for v in self.terms.obs_into.values()):
            raise ValueError("config.extra_actor_obs / extra_critic_obs reserve network inputs, but no observation term is routed into them "
                             "(extra_observations={name: (term, 'actor' | 'critic' | 'both')})")
        self.terms.bind(config.seed, rank, self.device, self.model_blob, self.nobs_actor, self.nobs_critic)
        self.traj = TrajBuffers(self.T, self.N, self.H, self.kcfg.depth, self.device, mirror=self.mirror, reward_comps=config.log_reward_components,
                                ld_actor=self.ld_actor, ld_critic=self.ld_critic, record_state=config.record_state,
                                terminal_value=bool(self.kcfg.gae_terminal_value))
        if self.kcfg.gae_terminal_value:        # the buffer kbj_rollout writes and kbj_gae reads (bootstrap_terminal_value)
            self.ctx.set_terminal_values(self.traj.value_term)
        # the statistics the device keeps over the rollouts, each switched on in the config (episode_stats, tracking_stats, gait_stats,
        # actuator_stats; host/episode.py, tracking.py, gait.py, actuator.py): the carrier's `acc` are the per-env rows next to the env state;
        # None means off. to_kbj() has refused actuator_stats without record_state
        N, dev, dt = self.N, self.device, config.ctrl_dt
        self.episodes = EpisodeStats(N, dt, config.log_reward_components, dev) if config.episode_stats else None
        self.tracking = TrackingStats(N, settle_steps(config.tracking_settle_seconds, dt), dev) if config.tracking_stats else None
        self.gait = GaitStats(N, dt, dev) if config.gait_stats else None
        self.actuator = ActuatorStats(N, levels_of_config(self.model_blob, config), dev, self.model_blob, dt) if config.actuator_stats else None
        # those that are on, in the order of the checkpoint members and of the scalar keys
        self._carriers = [c for c in (self.episodes, self.tracking, self.gait, self.actuator) if c is not None]
        self.opt_step = 0
        self.iteration = 0
        self._perm_gen = torch.Generator(device="cpu")
        self.ctx.env_reset_all(config.seed, self.traj.actor_obs[self.T], self.traj.critic_obs[self.T], self.traj.aux[self.T])

    # ---- reference API names (train.py:1059-1327, 1510-1572) ----
    def get_mujoco_model(self) -> L.Model:
        """train.py:1079-1081: the compiled robot (a kbj_model blob instead of mujoco.MjModel)."""
        return compiler.load_model(self.config.robot)

    def get_model(self, seed: int) -> torch.Tensor:
        """train.py:1278-1327: Model(actor, critic) as one flat fp32 vector in equinox leaf order."""
        p = torch.zeros(self.P, device=self.device)
        self.ctx.init_params(seed, p)
        return p

    def get_initial_model_carry(self) -> CarryBuffers:
        """train.py:1526-1543: zero LSTM carries and low-pass filter state."""
        return CarryBuffers(self.N, self.H, self.kcfg.depth, self.device, mirror=self.mirror)

    def sample_action(self, actor_obs, critic_obs, step_index: int, argmax: bool = False):
        """train.py:1545-1572 for all envs at one control step; returns (action, log_prob, value)."""
        a = torch.empty(self.N, L.NU, device=self.device)
        lp, v = torch.empty(self.N, device=self.device), torch.empty(self.N, device=self.device)
        self.ctx.policy_step(self.params, actor_obs, critic_obs, self.carry.c, self.config.seed, step_index, argmax, a, lp, v)
        return a, lp, v

    # ---- the hot path ----
    def rollout(self):
        """T control steps of all envs, trajectory + rewards on the device."""
        if self.terms:
            self._rollout_stepwise()
        else:
            self.ctx.rollout(self.params, self.carry.c, self.config.seed, self.iteration * self.T, self.traj.c)
        if self.extra_rewards:
            from .traj_view import apply_extra_rewards
            self.extra_reward_means = apply_extra_rewards(self.extra_rewards, self._extra_carries, self.trajectory(), self.traj.reward)
        for c in self._carriers:                  # behind the user rewards, so that the episodes count them (tracking and gait read the aux rows alone);
            c.after_rollout(self.ctx, self.traj.c)      # user terminations are in the DONE column already

    def _stats_vectors(self, carrier, cls):
        """(last, total) of `carrier` (copies) - or the refusal, when the switch of its class `cls` is off."""
        if carrier is None:
            raise B.KbjError(f"{cls.switch}_vectors() needs HumanoidWalkingTaskConfig.{cls.switch}=True")
        last, total = carrier.vectors()
        return last.copy(), total.copy()

    def _reduced_stats(self, carrier, cls, which) -> np.ndarray:
        """`carrier`'s vectors()[which] (which = None: both, stacked) over all ranks' envs: ONE StatsLayout.reduce, which every rank must
        call - or the refusal, when the switch of its class `cls` is off."""
        if carrier is None:
            raise B.KbjError(f"{cls.switch}() needs HumanoidWalkingTaskConfig.{cls.switch}=True")
        vec = np.stack(carrier.vectors()) if which is None else carrier.vectors()[which]
        if self.world_size > 1 or dist_util.FORCE_COLLECTIVE:
            vec = carrier.layout.reduce(torch.from_numpy(vec).to(self.device), self.world_size).cpu().numpy()
        return vec

    def _mode_stats(self, carrier, cls, total: bool) -> dict:
        """The last rollout's vector of `carrier`, or the totals', reduced over the ranks, as scalars under the prefix that goes with it."""
        vec = self._reduced_stats(carrier, cls, 1 if total else 0)
        return carrier.scalars(vec, cls.total_prefix if total else cls.prefix)

    def actuator_stats_vectors(self):
        """(last, total): this rank's raw KBJ_ACT vectors (float64 numpy, layout.ACT / AJNT) behind actuator_stats() - the rows of the last
        rollout and all since creation / resume."""
        return self._stats_vectors(self.actuator, ActuatorStats)

    def actuator_stats(self, total: bool = False, per_joint: bool = False):
        """What the policy asks of the motors (needs `actuator_stats=True` and `record_state=True` in the config) over the LAST rollout - or,
        with `total`, over all rollouts since the task was created or resumed, as `act_total/...`: per command mode that has rows
        `act/<mode>/power_abs_w`, `power_pos_w`, `cost_of_transport`, `torque_rms`, `at_torque_level_frac`, `at_stop_frac`,
        `action_rate_rms` / `_max`, `worst_joint`, `worst_joint_frac` (host/actuator.py actuator_scalars; the definitions: include/kbj.h
        kbj_actuator_stats). With `per_joint` instead the per-joint table of all rows together (actuator_joint_table: a dict per joint;
        `format_actuator_joint_table` renders it). In a multi-rank job the vectors are reduced over the ranks
        (dist.reduce_actuator_stats): every rank must call it."""
        if per_joint:
            return actuator_joint_table(self._reduced_stats(self.actuator, ActuatorStats, 1 if total else 0), self.model_blob, self.config.ctrl_dt)
        return self._mode_stats(self.actuator, ActuatorStats, total)

    def actuator_sweep(self, commands=None, repeats: int = 2, seconds: Optional[float] = None, seed_offset: int = 7919, **levels) -> list:
        """The actuator table: what the CURRENT policy asks of the motors under each of `commands` (as tracking_sweep takes them; default:
        host/tracking.default_command_grid). tracking_sweep's rollout - a context of its own with len(commands) * repeats envs (env e follows
        command e % K), `seconds` (default render_length_seconds) of argmax actions under a scripted Command term, with the state record of
        every step kept - then ONE kbj_actuator_stats call on a fresh carry with the per-env record. `levels`: keyword arguments of
        host/actuator.actuator_levels (default: the config's actuator_torque_level, actuator_speed_limit, actuator_stop_margin_deg; settings
        of this build, not of the reference). Returns one dict per command, pooled over its envs: `command`, `mode`, `power_abs_w`,
        `power_pos_w`, `cost_of_transport`, `torque_rms`, `at_torque_level_frac`, `at_stop_frac`, `action_rate_rms`, `worst_joint` (by name)
        and `worst_joint_frac` (its largest torque over its level), `failures_per_s` (nan over nothing). `format_actuator_table` renders
        it. Works with `actuator_stats` and `record_state` off. Like the gait and push tables, this one has NOT been taken on a trained
        policy."""
        return actuator_sweep(self, commands, repeats, seconds, seed_offset, **levels)[0]

    def gait_stats_vectors(self):
        """(last, total): this rank's raw KBJ_GAIT vectors (float64 numpy, layout.GAIT / GFOOT) behind gait_stats() - the rows of the last
        rollout and all since creation / resume."""
        return self._stats_vectors(self.gait, GaitStats)

    def gait_stats(self, total: bool = False) -> dict:
        """How the robot walks (needs `gait_stats=True` in the config) over the LAST rollout - or, with `total`, over all rollouts since the
        task was created or resumed, as `gait_total/...`: per command mode that has rows `gait/<mode>/double_support_frac`,
        `single_support_frac`, `flight_frac`, `step_rate_hz`, `repeat_frac` (hops), `torque_rms`, `torque_max`, per foot
        `left_` / `right_` `swing_s_mean` / `_std` / `_max`, `stance_s_mean` / `_std` / `_max`, `duty`, `clearance_m_mean` / `_max`,
        `force_n_mean` / `_max`, and `swing_asymmetry` (host/gait.py gait_scalars; the definitions: include/kbj.h kbj_gait_stats). In a
        multi-rank job the vectors are reduced over the ranks (dist.reduce_gait_stats): every rank must call it."""
        return self._mode_stats(self.gait, GaitStats, total)

    def gait_sweep(self, commands=None, repeats: int = 2, seconds: Optional[float] = None, seed_offset: int = 7919) -> list:
        """The gait table: how the CURRENT policy walks under each of `commands` (as tracking_sweep takes them; default:
        host/tracking.default_command_grid). tracking_sweep's rollout - a context of its own with len(commands) * repeats envs (env e follows
        command e % K), `seconds` (default render_length_seconds) of argmax actions under a scripted Command term, the user's Reset and
        network-input Observation terms applied as in validate(), Event terms not - then ONE kbj_gait_stats call on a fresh carry with the
        per-env record. Returns one dict per command, pooled over its envs: `command`, `mode`, per foot `left_` / `right_` `swing_s`,
        `stance_s` (mean, seconds), `clearance_m_mean` / `_max`, `force_n_max`; `step_rate_hz`, `double_support_frac` /
        `single_support_frac` / `flight_frac`, `repeat_frac`, `torque_rms`, `failures_per_s` (nan over nothing). `format_gait_table`
        renders it. Works with `gait_stats` off. Like the push table, this one has NOT been taken on a trained policy: what a
        good gait looks like in it is not known from this build."""
        return gait_sweep(self, commands, repeats, seconds, seed_offset)[0]

    def tracking_stats_vectors(self):
        """(last, total): this rank's raw KBJ_TRK vectors (float64 numpy, layout.TRK) behind tracking_stats() - the rows of the last rollout
        and all since creation / resume."""
        return self._stats_vectors(self.tracking, TrackingStats)

    def tracking_stats(self, total: bool = False) -> dict:
        """Command-tracking errors (needs `tracking_stats=True` in the config) of the LAST rollout - or, with `total`, of all rollouts since the
        task was created or resumed, as `track_total/...`: per command mode that has settled rows `track/<mode>/<err>_mean`, `_rms`, `_max`
        for lin_vel_err (m/s), yaw_rate_err (rad/s), tilt_err, height_err (m), arm_sq_err (rad^2) over the rows whose command has been held
        for `tracking_settle_seconds`, `rows_frac` (the mode's share of all rows) and `settled_frac`. In a multi-rank job the vectors are
        reduced over the ranks (dist.reduce_tracking_stats): every rank must call it."""
        return self._mode_stats(self.tracking, TrackingStats, total)

    def tracking_sweep(self, commands=None, repeats: int = 2, seconds: Optional[float] = None, settle_seconds: Optional[float] = None) -> list:
        """The joystick response table: how well the CURRENT policy follows each of `commands` ([K][<= 16] floats, missing components zero;
        default: host/tracking.default_command_grid - stand, the six directions at half and full range, one omni, one stand-bend command, from
        the config's command ranges). A validation-style context of K * repeats envs (env e follows command e % K) runs `seconds`
        (default render_length_seconds) with argmax actions through the step-wise loop, driven by a scripted Command term that hands every env
        its own command again after an in-episode reset; the user's Reset and network-input Observation terms apply as in validate(). One
        kbj_tracking_stats call then gives every row's errors. Returns one dict per command: `command`, `mode`, the five settled-row mean
        errors (per env over its rows whose command has been held for `settle_seconds`, default tracking_settle_seconds, then averaged over
        the repeats), `settled_rows` and `failures_per_s`. `format_tracking_table` renders it. Works with `tracking_stats` off. Every call
        creates a library context for its env count and length and closes it again (it is not cached as validate()'s is). Event terms
        (`extra_events`) do NOT run here: the table is about following the stick; push_sweep() is the one that shoves."""
        return tracking_sweep(self, commands, repeats, seconds, settle_seconds)[0]

    def push_sweep(self, forces=(50.0, 100.0, 150.0, 200.0), directions_deg=(0, 45, 90, 135, 180, 225, 270, 315), duration: float = 0.2, command=None,
                   push_at: float = 2.0, window: float = 3.0, hold: float = 0.5, tolerances: Optional[dict] = None, repeats: int = 4, torque=None,
                   seed_offset: int = 7919):
        """The robustness table: what push the CURRENT policy survives and how fast it is back on its command. One case per (force in N,
        direction in degrees): a horizontal shove of `duration` seconds at the base, its direction in the robot's HEADING frame at the moment
        of the push (0 = from behind, pushing it forward; 90 = to its left), plus `torque` (N m, same frame) if given. A context of its own
        with len(forces) * len(directions_deg) * repeats envs (env e runs case e % cases; at most 256 cases) holds `command` (default: stand)
        with argmax actions through the step-wise loop; the Event term host/push.ScriptedPush switches the built-in push event off (again
        after every in-episode reset) and applies every env's push at row round(push_at / ctrl_dt); the user's Reset and network-input
        Observation terms apply as in validate(), other Event terms and the Command term do not. kbj_tracking_stats then gives every row's
        errors and kbj_push_recovery the outcome per env and the statistics per case: a push is VOID when the env was not within the
        tolerances for `hold` seconds before it (or had just been reset); otherwise the env FELL, RECOVERED (within the tolerances for
        `hold` seconds, inside `window` seconds after the push ended), stayed UNRECOVERED, or was CENSORED by a time-out. `tolerances`
        ({error name: bound}, constants.TRACKING_ERROR_NAMES; missing names keep host/push.DEFAULT_TOLERANCES) are SETTINGS, echoed in every
        entry - not measured thresholds. Returns (entries, record): per case the settings, `valid` pushes and `void` count, `fell_frac` /
        `recovered_frac` / `unrecovered_frac` / `censored_frac` of the valid ones, `recovery_s_mean` / `_max`, `peak_tilt_mean` / `_max`,
        `peak_lin_vel_err_mean` / `_max` (nan over nothing); and the PushRecord of the device data. `format_push_table` renders the entries."""
        return push_sweep(self, forces, directions_deg, duration, command, push_at, window, hold, tolerances, repeats, torque, seed_offset)

    def step_sweep(self, transitions=None, step_at: float = 3.0, window: float = 4.0, hold: float = 0.5, smooth: float = 0.5, rise_level: float = 0.9,
                   band_frac: float = 0.1, band_abs=(0.15, 0.15, 0.25), min_step=(0.05, 0.05, 0.05), repeats: int = 4, seed_offset: int = 7919):
        """The step-response table: what the CURRENT policy does when the stick MOVES. One case per transition (from command, to command;
        [<= 16] floats each, missing components zero; default: host/step.default_step_grid - starts, stops, a speed-up, the reversal and a
        turn reversal at the config's full command ranges). A context of its own with len(transitions) * repeats envs (env e runs case
        e % cases; at most 256 cases) and round(step_at / ctrl_dt) + round(window / ctrl_dt) rows runs argmax actions through the step-wise
        loop under the Command term host/step.SteppedCommand: every env holds its old command until row round(step_at / ctrl_dt) and its new
        one from there on, again after every in-episode reset; the user's Reset and network-input Observation terms apply as in validate(),
        Event terms do not. ONE kbj_step_response call then scores every env on the device, with one group per case: per channel (forward
        and sideways velocity in the robot's heading frame, yaw rate), smoothed over `smooth` seconds (at most 32 rows), a step is VOID when
        the env was not inside the band of its OLD command (or had just been reset) when the stick moved; otherwise the env FELL, SETTLED
        (every channel inside max(band_abs, band_frac x step size) of the new command for `hold` seconds, inside `window` seconds), stayed
        UNSETTLED, or was CENSORED by a time-out. Beside that: the rise time to `rise_level` of the step, the overshoot, the cross-coupling
        into the channels whose command moved by less than `min_step`, and the travel until settled - the stopping distance of a stop; it
        is a path integral in the heading frame and a displacement only while the heading barely turns. All of these are SETTINGS, echoed
        in every entry - not measured thresholds. Returns (entries, record): per case the settings and host/step.case_summary's figures
        (nan over nothing), and the StepRecord of the device data. `format_step_table` renders the entries. Like the push and gait
        tables, this one has NOT been taken on a trained policy."""
        return step_sweep(self, transitions, step_at, window, hold, smooth, rise_level, band_frac, band_abs, min_step, repeats, seed_offset)

    def frequency_sweep(self, points=None, periods=None, cycles: int = 4, min_window: float = 4.0, start_at: float = 2.0, settle: float = 2.0,
                        min_amp=(0.05, 0.05, 0.05), repeats: int = 4, seed_offset: int = 7919):
        """The frequency-response table: how the CURRENT policy follows a stick that KEEPS MOVING. One case per (operating point, period):
        an operating point is (base command [<= 16] floats, channel 0 forward / 1 sideways / 2 yaw, amplitude; default:
        host/frequency.default_frequency_points - each channel around standing at half its range, forward around half speed at a quarter),
        a period is an int in rows (a multiple of 4 in [4, 256]) or a float frequency in Hz, snapped to P = 4 round(1 / (4 f ctrl_dt))
        (default 200, 100, 48, 24, 12, 8 rows: 0.25 to 6.25 Hz at 50 Hz control). A context of its own with cases * repeats envs (env e
        runs case e % cases; at most 256 cases) runs argmax actions through the step-wise loop under the Command term
        host/frequency.SineCommand: from row round(start_at / ctrl_dt) on the driven word is base + amplitude cos(2 pi (row - start) / P),
        again after every in-episode reset; the user's Reset and network-input Observation terms apply as in validate(), Event terms do
        not. After ceil(settle / (P ctrl_dt)) whole periods, K = max(cycles, ceil(min_window / (P ctrl_dt))) whole periods are measured:
        ONE kbj_frequency_response call, with one group per case, sums every response channel against the recorded command and against
        the same command a quarter period earlier. A window is VOID when an episode ended in the quarter period in front of it; otherwise
        the env FELL, was CENSORED by a time-out, left a FLAT window (the recorded command swung by less than `min_amp`) or a MEASURED
        one. From the sums pooled over a case's MEASURED envs the host forms gain, gain in dB, lag in degrees, delay in ms, coherence
        and the cross-coupling gain into the two channels that were not driven (host/frequency.case_summary), and per operating point
        the -3 dB bandwidth by interpolation over log f (`bandwidth_hz`; `bandwidth_below_range` when the gain is below -3 dB already at
        the lowest frequency). `min_amp` and the grid are SETTINGS, echoed in every entry - not measured thresholds - and the figures
        are linear-systems language applied to a nonlinear walker: the coherence says how far to trust them. Returns (entries, record):
        per case the settings and figures (nan over nothing), and the FrequencyRecord of the device data. `format_frequency_table` renders
        the entries. Like the step table, this one has NOT been taken on a trained policy."""
        return frequency_sweep(self, points, periods, cycles, min_window, start_at, settle, min_amp, repeats, seed_offset)

    def robustness_sweep(self, perturbations=None, commands=None, repeats: int = 8, seconds: Optional[float] = None, settle_seconds: Optional[float] = None,
                         seed_offset: int = 7919):
        """The model-robustness table: what the CURRENT policy does on a robot that is NOT the model it trained on. One case per
        (perturbation, command): a host/robustness.Perturbation names how the model row differs - mass, a payload on the torso, floor
        friction, armature, joint friction, action latency, a COM shift, and per joint (or per leg / arm) kp, kd, torque limit and action
        bias; default: host/robustness.default_perturbations, 16 cases around and beyond the randomisers' ranges, SETTINGS of this build
        and not measured thresholds - and a command is [<= 16] floats (default: stand, forward at half and full range, turn left at full
        range). A context of its own with cases * repeats envs (env e runs case e % cases; at most 256 cases) runs `seconds` (default
        render_length_seconds) of argmax actions through the step-wise loop under a scripted Command term; kbj_env_perturb writes every
        env's record on row 0 and again, behind every step, on the envs whose episode has just started (an in-step reset redraws the
        model row); the user's Reset and network-input Observation terms apply as in validate(), Event terms do not. kbj_tracking_stats
        then gives every row's errors and ONE kbj_robustness call, with one group per case, the falls and the settled-row errors.
        Returns (entries, record): per case `perturbation`, `changed` (its non-default fields), `command`, `mode`, `in_training_range`
        (host/robustness.in_training_range: every knob inside what the randomisers draw), `envs`, `survival` (the share of envs that
        never fell), `falls_per_s`, `first_fall_s_mean` / `first_fall_s_min`, `timeouts`, the five settled-row mean errors (rows whose
        command has been held for `settle_seconds`, default tracking_settle_seconds) and `settled_rows` (nan over nothing); and the
        RobustnessRecord of what the run left behind. A refused perturbation raises ValueError naming its field before the device is
        touched. `format_robustness_table` renders the entries. Like the push, gait, step and frequency tables, this one has NOT been
        taken on a trained policy."""
        return robustness_sweep(self, perturbations, commands, repeats, seconds, settle_seconds, seed_offset)

    def episode_stats_vectors(self):
        """(last, total): this rank's raw KBJ_EPST vectors (float64 numpy, layout.EPST) behind episode_stats() - the episodes that finished in
        the last rollout and all since creation / resume."""
        return self._stats_vectors(self.episodes, EpisodeStats)

    def episode_stats(self) -> dict:
        """Episode metrics (needs `episode_stats=True` in the config): `episode/...` over the episodes that finished in the LAST rollout,
        `episode_total/...` over all that finished since the task was created or resumed - count, return mean / std / min / max, length
        and time to failure in seconds, fractions per termination cause and, with `log_reward_components`, the mean episodic sum of every
        reward term. In a multi-rank job the vectors are reduced over the ranks (dist.reduce_episode_stats): every rank must call it."""
        last, total = self._reduced_stats(self.episodes, EpisodeStats, None)      # both from one stacked reduce
        return {**self.episodes.scalars(last, EpisodeStats.prefix), **self.episodes.scalars(total, EpisodeStats.total_prefix)}

    def trajectory(self):
        """The last rollout as the Python reward terms see it: with `config.record_state` a ksim-shaped `host.trajectory.Trajectory`
        (trajectory.qpos / .qvel / .xpos / .xquat / .ctrl / .done / .obs[...] / .command["unified_command"], train.py:138-506), else the
        `TrajectoryView` of the aux record. User observation terms appear under their names in `.obs` / `.extra_observations`."""
        extra = {k: v[:self.T] for k, v in self.extra_obs_buffers.items()}
        if self.config.record_state:
            from .trajectory import Trajectory
            view = Trajectory(self.traj, self.T, self.model_blob, extra_observations=extra)
        else:
            from .traj_view import TrajectoryView
            view = TrajectoryView(self.traj, self.T)
        view.extra_observations = extra
        return view

    def _rollout_stepwise(self):
        """kbj_rollout's steps as separate ABI calls with the user's terms between the env step and the carry reset (host/user_terms.py)."""
        T, tr, c, terms = self.T, self.traj, self.ctx, self.terms
        tr.actor_obs[0].copy_(tr.actor_obs[T]); tr.critic_obs[0].copy_(tr.critic_obs[T]); tr.aux[0].copy_(tr.aux[T])   # row T of the last rollout is row 0 of this one
        tr.carry0_actor_hc.copy_(self.carry.actor_hc); tr.carry0_critic_hc.copy_(self.carry.critic_hc); tr.carry0_lpf.copy_(self.carry.lpf)
        if self.mirror:
            tr.carry0_actor_mirror_hc.copy_(self.carry.actor_mirror_hc); tr.carry0_critic_mirror_hc.copy_(self.carry.critic_mirror_hc)
            tr.carry0_lpf_mirror.copy_(self.carry.lpf_mirror)
        first = self.iteration * T              # the terms' step index is iteration * T + row
        for buf in self.extra_obs_buffers.values():
            buf[0].copy_(buf[T])
        if not terms.started:                   # the state and the rows env_reset_all wrote: every env starts an episode, the user columns are zero
            terms.run_hooks(c, tr, 0, first, [terms.apply_resets, terms.apply_events, terms.apply_command, terms.observe])
            terms.started = True
        terms.run_steps(c, tr, self.carry, self.params, T, seed=self.config.seed, first_step=first, argmax=False, first_index=first,
                        hooks=[terms.apply_terminations, terms.apply_resets, terms.apply_events, terms.apply_command, terms.observe],
                        terminal=bool(self.kcfg.gae_terminal_value))
        if self.kcfg.gae_tail_value:          # V(s_T) for GAE, as kbj_rollout computes it: row T, the carries the last reset left, the rollout's parameters
            c.critic_value(self.params, tr.critic_obs[T], self.carry.c, tr.value_tail)
        c.rewards(tr.aux, T, tr.reward, tr.comps)

    def update(self):
        """GAE, then num_passes x (N / B) minibatch steps: BPTT gradient, all-reduce, AdamW."""
        # the passes' permutations: drawn on the host (same streams as the oracle trainer), staged in pinned memory and uploaded with
        # stream-ordered copies BEFORE anything of the update is enqueued - a pageable `.to(device)` per pass blocks the host until the
        # queued work has drained and leaves the GPU idle (~0.3 ms) while the next minibatch is being enqueued
        npass = self.kcfg.num_passes
        if self._perm_pinned is None or self._perm_pinned.shape != (npass, self.N):
            self._perm_pinned = torch.empty(npass, self.N, dtype=torch.int32).pin_memory()
            self._perm_dev = torch.empty(npass, self.N, dtype=torch.int32, device=self.device)
            self._perm_event = torch.cuda.Event()
        else:
            self._perm_event.synchronize()       # the previous upload has left the staging buffer (it has, unless the caller never syncs)
        for p in range(npass):
            self._perm_gen.manual_seed((self.config.seed * 1000003 + self.iteration * 97 + p) & 0x7FFFFFFF)
            self._perm_pinned[p].copy_(torch.randperm(self.N, generator=self._perm_gen))
        self._perm_dev.copy_(self._perm_pinned, non_blocking=True)
        self._perm_event.record()
        self.ctx.gae(self.traj.c, self.traj.adv, self.traj.target)
        for p in range(npass):
            perm = self._perm_dev[p]
            nmb = self.N // self.B
            per_pass = self.config.allreduce == "per_pass"
            if per_pass:
                self.grad_acc.zero_()
            for mb in range(nmb):
                idx = perm[mb * self.B:(mb + 1) * self.B].contiguous()
                if self.config.global_advantage_stats:
                    self._adv_sums = dist_util.global_advantage_sums(self.traj.adv.index_select(1, idx.long()), self.world_size)   # kept alive until the call has run
                    self.ctx.set_advantage_sums(self._adv_sums)
                self.ctx.ppo_grad(self.params, self.traj.c, idx, self.B, self.traj.adv, self.traj.target, self.grad, self.metrics)
                # next-minibatch hint: its parameter-independent gathers run under this minibatch's exchange + optimizer step
                nxt = perm[(mb + 1) * self.B:(mb + 2) * self.B] if mb + 1 < nmb else (self._perm_dev[p + 1][:self.B] if p + 1 < npass else None)
                if nxt is not None and not _NO_PREFETCH:
                    self.ctx.ppo_prefetch(self.traj.c, nxt.contiguous())
                if per_pass:
                    self.grad_acc.add_(self.grad)          # kbj_ppo_grad overwrites `grad`; the pass total lives in grad_acc
                    if mb + 1 < nmb:
                        continue
                g = self.grad_acc if per_pass else self.grad
                if self.config.overlap_allreduce and not per_pass:
                    if self._comm_stream is None:
                        self._comm_stream = torch.cuda.Stream(device=self.device)
                    scale = dist_util.allreduce_grad_overlapped_(self.ctx, g, self.ctx.actor_param_count(), self.world_size, self._comm_stream)
                else:
                    scale = dist_util.allreduce_grad_(g, self.world_size)   # RCCL over xGMI: the one exchange step
                if per_pass:
                    scale /= nmb                                     # mean over the pass's minibatches (and ranks)
                if self.config.use_lr_decay:
                    lr = cosine_decay_lr(self.config, self.opt_step)
                    if self.config.adam_weight_decay == 0.0:      # train.py:1074-1075 as written: no sign flip behind scale_by_adam
                        if not self._warned_ascent:
                            warnings.warn("use_lr_decay with adam_weight_decay == 0 reproduces train.py:1074-1075 as written: "
                                          "optax.chain(scale_by_adam, scale_by_schedule) has no sign flip, the update ASCENDS the loss")
                            self._warned_ascent = True
                        lr = -lr
                    self.ctx.set_learning_rate(lr)
                self.opt_step += 1
                self.ctx.adamw_step(self.params, self.opt_m, self.opt_v, g, self.opt_step, scale)

    def train_iteration(self):
        self.rollout()
        self.update()
        self.iteration += 1
        self.ctx.synchronize()   # one sync per iteration: surfaces device-side errors (e.g. a recurrence hand-off timeout) as KbjError

    def env_steps_per_iteration(self) -> int:
        return self.N * self.T

    # ---- read-only views of the compiled task wiring, under the reference's method names (train.py:1059-1276) ----
    def get_optimizer(self) -> wiring.OptimizerSpec:
        """train.py:1059-1077: adam / adamw, optionally under a cosine decay schedule; executed by kbj_adamw_step."""
        return wiring.optimizer(self.config, self.kcfg)

    def get_mujoco_model_metadata(self, mj_model: Optional[L.Model] = None) -> dict:
        """train.py:1083-1089: per-joint kp / kd / soft torque limit of metadata.json (compiled into the model blob)."""
        m = mj_model or self.model_blob
        return {n: dict(kp=m.kp[i], kd=m.kd[i], soft_torque_limit=m.tau_limit[i]) for i, n in enumerate(constants.JOINT_NAMES)}

    def get_actuators(self) -> wiring.PositionActuatorsSpec:
        return wiring.actuators(self.model_blob, self.kcfg)

    def get_physics_randomizers(self) -> dict:
        return wiring.physics_randomizers(self.kcfg)

    def get_events(self) -> dict:
        """train.py:1134-1144: the built-in ForcePushEvent as a frozen view, then the user's Event terms (`extra_events`) under their names."""
        return {**wiring.events(self.kcfg), **self.terms.events}

    def get_resets(self) -> list:
        return wiring.resets(self.kcfg)

    def get_observations(self) -> dict:
        return wiring.observations(self.kcfg)

    def get_commands(self) -> dict:
        return wiring.commands(self.model_blob, self.kcfg)

    def get_rewards(self) -> dict:
        return wiring.rewards(self.kcfg)

    def get_terminations(self) -> dict:
        return wiring.terminations(self.kcfg)

    def get_curriculum(self) -> wiring.CurriculumSpec:
        return wiring.CurriculumSpec()

    def get_ppo_variables(self, trajectory: Optional[TrajBuffers] = None, params: Optional[torch.Tensor] = None) -> dict:
        """train.py:1510-1524. Without arguments: the variables of the LAST rollout as its own policy steps produced them (ksim recomputes
        them with the pre-update model in a separate on-policy pass: same parameters, same observations). With `trajectory` (any
        TrajBuffers of this task's shape - e.g. a reloaded one, or the last rollout after the parameters changed) and optionally
        `params`: that separate pass itself (kbj_ppo_forward: both nets through the T steps from the trajectory's start carries, carry
        reset where done, no gradients), minibatch by minibatch. Returns PPOVariables' per-step fields as [T][N](x20) tensors."""
        if trajectory is None:
            return dict(log_probs=self.traj.logp, values=self.traj.value, action=self.traj.action)
        p = self.params if params is None else params
        T, N, B, dev = self.T, self.N, self.B, self.device
        out = dict(log_probs=torch.empty(T, N, device=dev), values=torch.empty(T, N, device=dev), entropy=torch.empty(T, N, device=dev),
                   action_std=torch.empty(T, N, L.NU, device=dev), action_mean=torch.empty(T, N, L.NU, device=dev))
        lp, v, en = (torch.empty(T, B, device=dev) for _ in range(3))
        sd, mu = torch.empty(T, B, L.NU, device=dev), torch.empty(T, B, L.NU, device=dev)
        for mb in range(N // B):
            idx = torch.arange(mb * B, (mb + 1) * B, device=dev, dtype=torch.int32)
            self.ctx.ppo_forward(p, trajectory.c, idx, B, lp, v, en, sd, mu)
            sl = slice(mb * B, (mb + 1) * B)
            out["log_probs"][:, sl], out["values"][:, sl], out["entropy"][:, sl] = lp, v, en
            out["action_std"][:, sl], out["action_mean"][:, sl] = sd, mu
        out["action"] = trajectory.action
        return out

    def run_actor(self, actor_obs: torch.Tensor, critic_obs: torch.Tensor, step_index: int = 0):
        """train.py:1351-1379 + Actor.forward (:913-941) for all envs: returns the distribution's mode (filtered mean incl. biases).
        Both nets advance their carries (kbj_policy_step is the fused actor + critic step)."""
        a, _, _ = self.sample_action(actor_obs, critic_obs, step_index, argmax=True)
        return a

    def run_critic(self, actor_obs: torch.Tensor, critic_obs: torch.Tensor, step_index: int = 0):
        """train.py:1381-1433 + Critic.forward (:993-1004): the value estimate (carries advance as in run_actor)."""
        _, _, v = self.sample_action(actor_obs, critic_obs, step_index, argmax=True)
        return v

    # ---- checkpointing in the xax `ckpt.bin` layout (host/ckpt.py; convert.sh:4, train.py:1788) ----
    def save_checkpoint(self, path: str, background: bool = False):
        """Everything a bit-exact resume needs: parameters, optimizer, counters (upstream members) + env rows, reward carries, model
        carries and the pending observation rows (kbj_* members). The device arrays are copied to the host here, synchronously (a
        consistent snapshot: ~150 MB at 8192 envs); with `background` the container (npy blobs, gzip, fsync, rename) is written by a
        thread while training goes on - `wait_for_checkpoint()` joins it, and a new save waits for the previous one first. launch() saves
        this way: written in line a save costs seconds of a loop that runs an iteration in a third of one."""
        self.wait_for_checkpoint()
        T = self.T
        ep, es = self.ctx.env_get_state()
        extras = dict(ep=ep, es=es, rc=self.ctx.env_get_reward_carry(), actor_hc=self.carry.actor_hc.cpu().numpy(), critic_hc=self.carry.critic_hc.cpu().numpy(),
                      lpf=self.carry.lpf.cpu().numpy(), actor_obs_T=self.traj.actor_obs[T].cpu().numpy(), critic_obs_T=self.traj.critic_obs[T].cpu().numpy(),
                      aux_T=self.traj.aux[T].cpu().numpy())
        if self.mirror:
            extras.update(actor_mirror_hc=self.carry.actor_mirror_hc.cpu().numpy(), critic_mirror_hc=self.carry.critic_mirror_hc.cpu().numpy(),
                          lpf_mirror=self.carry.lpf_mirror.cpu().numpy())
        for c in self._carriers:
            extras.update(c.checkpoint_state())
        # carries of Python StatefulReward terms (extra_rewards): tensors (or tuples / lists of tensors) per term name
        for name, carry in self._extra_carries.items():
            leaves = list(carry) if isinstance(carry, (tuple, list)) else [carry]
            for i, leaf in enumerate(leaves):
                extras[f"extra_{name}_{i}"] = leaf.detach().cpu().numpy() if hasattr(leaf, "detach") else np.asarray(leaf)
            extras[f"extra_{name}_n"] = np.asarray(len(leaves) if isinstance(carry, (tuple, list)) else 0, np.int32)   # 0: a bare tensor
        cfg = dataclasses.asdict(self.config)
        cfg["action_latency_range"] = list(cfg["action_latency_range"])
        if cfg.get("fixed_command") is not None:
            cfg["fixed_command"] = list(cfg["fixed_command"])
        state = dict(num_steps=self.iteration, opt_step=self.opt_step, num_samples=self.iteration * self.N * self.T * self.world_size,
                     rank=self.rank, world_size=self.world_size)
        args = (path, self.params.cpu().numpy(), self.opt_m.cpu().numpy(), self.opt_v.cpu().numpy(), self.opt_step, self.H, self.kcfg.depth, state, cfg, extras)
        kw = dict(schedule_count=self.opt_step if self.config.use_lr_decay else None, extra_obs=self.extra_obs)
        if not background:
            ckpt_io.save_ckpt(*args, **kw)
            return

        def write():
            try:
                ckpt_io.save_ckpt(*args, **kw)
            except BaseException as e:      # surfaced by wait_for_checkpoint(): a failed save must not pass silently
                self._save_error = e
        self._save_error = None
        self._save_thread = threading.Thread(target=write, name="kbj-ckpt-writer", daemon=False)
        self._save_thread.start()

    def wait_for_checkpoint(self):
        """Join a background save_checkpoint(); re-raises what the writer raised."""
        if self._save_thread is not None:
            self._save_thread.join()
            self._save_thread = None
            err, self._save_error = self._save_error, None
            if err is not None:
                raise err

    def load_checkpoint(self, path: str):
        """Resume from save_checkpoint(): the next train_iteration() is bit-identical to the one the saved run would have made."""
        z = ckpt_io.load_ckpt(path, "all", hidden_size=self.H, depth=self.kcfg.depth)
        dev = self.device
        self.params.copy_(torch.from_numpy(z["model"]))
        opt, st = z["opt_state"], z["state"]
        if opt is not None:
            self.opt_m.copy_(torch.from_numpy(opt["mu"])); self.opt_v.copy_(torch.from_numpy(opt["nu"]))
            # `opt_step` is this build's key; an upstream checkpoint only has the optax `count` leaf (and xax's num_steps)
            self.opt_step = int(st.get("opt_step", opt["count"]))
        else:
            # no optimizer member, or one this build cannot map onto (mu, nu): the moments restart from zero, and so must the step count -
            # Adam's bias correction at the OLD count on empty moments would be ~1 instead of 1 / (1 - beta^t) and shrink the first steps
            self.opt_m.zero_(); self.opt_v.zero_()
            self.opt_step = 0
            if ckpt_io.has_member(path, "opt_state_0"):
                warnings.warn(f"{path}: opt_state_0 is present but does not map onto (count, mu, nu) of this model - "
                              "resuming with FRESH Adam moments and optimizer step 0 (parameters were loaded)")
        self.iteration = int(st.get("num_steps", 0))
        # a resumed run's row 0 already carries the user observation columns and the user command term's commands, its env rows the user Reset terms' state
        self.terms.started = self.iteration > 0
        x = z["extras"]
        for c in self._carriers:
            c.load_checkpoint_state(x)
        if "es" not in x:
            return            # a model-only checkpoint (e.g. written by the reference): parameters and optimizer only
        if x["es"].shape[0] != self.N:
            raise B.KbjError(f"checkpoint holds {x['es'].shape[0]} envs, this task has {self.N}")
        self.ctx.env_set_state(x["ep"], x["es"])
        self.ctx.env_set_reward_carry(x["rc"])
        T = self.T
        self.carry.actor_hc.copy_(torch.from_numpy(x["actor_hc"])); self.carry.critic_hc.copy_(torch.from_numpy(x["critic_hc"]))
        self.carry.lpf.copy_(torch.from_numpy(x["lpf"]))
        self.traj.actor_obs[T].copy_(torch.from_numpy(x["actor_obs_T"])); self.traj.critic_obs[T].copy_(torch.from_numpy(x["critic_obs_T"]))
        self.traj.aux[T].copy_(torch.from_numpy(x["aux_T"]))
        if self.mirror:
            self.carry.actor_mirror_hc.copy_(torch.from_numpy(x["actor_mirror_hc"]))
            self.carry.critic_mirror_hc.copy_(torch.from_numpy(x["critic_mirror_hc"]))
            self.carry.lpf_mirror.copy_(torch.from_numpy(x["lpf_mirror"]))
        self._extra_carries = {}
        for name in self.extra_rewards:      # Python StatefulReward carries; a term the checkpoint does not know starts from initial_carry
            if f"extra_{name}_n" in x:
                n = int(x[f"extra_{name}_n"])
                leaves = [torch.from_numpy(np.array(x[f"extra_{name}_{i}"])).to(dev) for i in range(max(n, 1))]
                self._extra_carries[name] = tuple(leaves) if n > 0 else leaves[0]

    @classmethod
    def load_task(cls, ckpt_path: str, device: Optional[torch.device] = None) -> "HumanoidWalkingTask":
        """convert.py:36 `HumanoidWalkingTask.load_task(ckpt_path)`: rebuild the task from the checkpoint's config member and
        load its state."""
        cfg = ckpt_io.load_ckpt(ckpt_path, "config")
        fields = {f.name for f in dataclasses.fields(HumanoidWalkingTaskConfig)}
        kw = {k: v for k, v in cfg.items() if k in fields}
        for k in ("action_latency_range", "fixed_command"):
            if kw.get(k) is not None:
                kw[k] = tuple(kw[k])
        task = cls(HumanoidWalkingTaskConfig(**kw), device=device)
        task.load_checkpoint(ckpt_path)
        return task

    def load_ckpt(self, path: str, init_params=None, part: str = "model"):
        """convert.py:39 `task.load_ckpt(ckpt_path, init_params=..., part="model")[0]`: returns a 1-tuple-like list whose first element is
        the requested part; for "model" a ModelView with `.actor` (named leaves) as convert.py:44-46 reads it."""
        if part == "model":
            flat = ckpt_io.load_ckpt(path, "model", hidden_size=self.H, depth=self.kcfg.depth)
            return [ModelView(flat, self.H, self.kcfg.depth, self.extra_obs)]
        return [ckpt_io.load_ckpt(path, part, hidden_size=self.H, depth=self.kcfg.depth)]

    # ---- validation (train.py:1564 argmax=True; valid_every_n_steps train.py:1789) ----
    def validate(self, num_envs: int = 64, seconds: Optional[float] = None, seed_offset: int = 7919, _capture=None, _stepwise: bool = False) -> dict:
        """Deterministic validation rollout: a separate small env set (its own context, carries and buffers, so training state is
        untouched), actions = the distribution's mode, `render_length_seconds` long. Returns scalar statistics.
        User Reset / Event / Command / Observation terms are applied as in training; user TERMINATION terms (`extra_terminations`) are NOT - validation
        episodes end by the built-in terminations (bad z, tilt, episode length) only, on the fused and on the step-wise path alike.
        `_capture(ctx, frame)` (view()): called after the reset (frame 0) and after every control step."""
        seconds = self.config.render_length_seconds if seconds is None else seconds
        T = max(1, int(round(seconds / self.config.ctrl_dt)))
        key, terms = (num_envs, T), self.terms
        if self._valid is None or self._valid.key != key:
            vcfg = self.config.to_kbj(num_envs) if num_envs % self.config.batch_size == 0 else dataclasses.replace(self.config, batch_size=num_envs).to_kbj(num_envs)
            vcfg.rollout_len = T
            vcfg.gae_bootstrap_truncation = vcfg.gae_tail_value = vcfg.gae_terminal_value = 0      # validation never runs GAE: no tail pass, no carry copy, no terminal rows
            if terms.command_term is not None:
                vcfg.command_mode = 1
            vctx = B.Context(self.model_blob, vcfg, self.device.index or 0, torch.cuda.current_stream().cuda_stream)
            self._valid = _Validation(key, vctx, CarryBuffers(num_envs, self.H, self.kcfg.depth, self.device, mirror=self.mirror),
                                      TrajBuffers(T, num_envs, self.H, self.kcfg.depth, self.device, mirror=self.mirror, reward_comps=True,
                                                  ld_actor=self.ld_actor, ld_critic=self.ld_critic, record_state=self.actuator is not None))
        _, vctx, carry, tr = self._valid
        seed = self.config.seed + seed_offset
        carry.zero_()
        terms.event_state_of(vctx).clear()      # every validation starts its Event terms afresh, in a state of its own (the context's): training's is untouched
        vctx.env_reset_all(seed, tr.actor_obs[0], tr.critic_obs[0], tr.aux[0])
        # the user's Reset and Command terms shape and drive the validation episodes as they do the training ones; of the Observation terms
        # only those that are network inputs matter here (they drive the validation policy too). The terms' step index is seed_offset + row.
        feeds = any(self.extra_obs)
        terms.run_hooks(vctx, tr, 0, seed_offset, [terms.apply_resets, terms.apply_events, terms.apply_command] + ([terms.observe_rows] if feeds else []))
        if _capture is not None:
            _capture(vctx, 0)
        if _capture is None and not feeds and terms.command_term is None and not terms.resets and not terms.events and not _stepwise:
            # no user term and nothing to capture between the steps: ONE kbj_rollout call in argmax mode (the same kernels, bit-identical to the
            # step-by-step loop below, ~3 x fewer host calls: 0.05 instead of 0.15 s for 64 envs x 500 steps). kbj_rollout takes its first
            # observation from row T (the previous rollout's last), so the reset rows move there first.
            tr.actor_obs[T].copy_(tr.actor_obs[0]); tr.critic_obs[T].copy_(tr.critic_obs[0]); tr.aux[T].copy_(tr.aux[0])
            vctx.set_rollout_argmax(True)
            try:
                vctx.rollout(self.params, carry.c, seed, 0, tr.c)
            finally:
                vctx.set_rollout_argmax(False)      # the cached context samples again whatever happened (the flag is context state, not a call argument)
        else:
            # NOT training's order (terminations, resets, command, observations): here the observations come BEFORE the command, so an Observation
            # term that reads the command columns of the row being written sees the previous command where training shows it the new one.
            # Kept as it is; unifying the two is a behaviour change of its own.
            hooks = [terms.apply_resets, terms.apply_events] + ([terms.observe_rows] if feeds else []) + [terms.apply_command]
            if _capture is not None:
                hooks.append(lambda s: _capture(vctx, s.row))
            terms.run_steps(vctx, tr, carry, self.params, T, seed=seed, first_step=0, argmax=True, first_index=seed_offset, hooks=hooks)
            vctx.rewards(tr.aux, T, tr.reward, tr.comps)
        # the same kernels on the validation trajectory, on the fused and on the step-wise path: every validation starts its episodes and carries afresh
        vecs = [c.fresh(vctx, tr.c, num_envs, self.device, *c.settings) for c in self._carriers]
        vctx.synchronize()
        done = tr.done
        fails, succ = float((done < 0).sum()), float((done > 0).sum())
        out = {"valid/reward_per_step": float(tr.reward.mean()), "valid/failures_per_step": fails / (T * num_envs),
               "valid/episode_length_s": float(T * num_envs / max(1.0, fails + succ + num_envs) * self.config.ctrl_dt), "valid/value_mean": float(tr.value.mean())}
        for name, v in zip(constants.REWARD_NAMES, tr.comps.mean(dim=(0, 1)).cpu().tolist()):
            out[f"valid/reward/{name}"] = v
        for c, vec in zip(self._carriers, vecs):
            out.update(c.valid_scalars(vec.cpu().numpy()))
        return out

    def close_validation(self):
        """Drop the cached validation / view context (its env rows, workspace and lanes). validate() builds it again on demand. Measured on
        MI355X (tools/validate_cliff.py, 8192 envs): keeping it costs the training iterations nothing (365.2 ms before the first validation,
        366.1 / 365.3 / 364.8 ms after a validation, a second one and a view), re-creating it costs 0.15 s per validation - so it stays cached."""
        if self._valid is not None:
            self._valid.ctx.close()
            self._valid = None

    def close(self):
        """Release the library contexts of this task (training and validation)."""
        self.wait_for_checkpoint()
        self.close_validation()
        self.ctx.close()

    def view(self, path: Optional[str] = None, num_envs: int = 4, seconds: Optional[float] = None, seed_offset: int = 7919):
        """`run_mode=view` (reference README.md:66-70; train.py:1783-1784 render_track_body_id / render_length_seconds): the validation
        rollout above on `num_envs` envs with the generalised positions recorded after every control step (kbj_env_get_state), returned
        as a `host.view.Recording`; with `path` (a stem) also written as `<path>.npz` and a self-contained `<path>.html` player."""
        from .view import Recording
        frames, eps = [], []

        def capture(vctx, frame):
            ep, es = vctx.env_get_state()
            frames.append(es[:, L.ES["QPOS"]:L.ES["QPOS"] + int(self.model_blob.nq)].copy())
            if frame == 0:
                eps.append(ep.copy())
        stats = self.validate(num_envs, seconds, seed_offset, _capture=capture)
        tr = self._valid.traj
        T = len(frames) - 1
        rec = Recording(self.model_blob, np.stack(frames), eps[0], tr.aux[:T + 1, :, L.AUX["CMD"]:L.AUX["CMD"] + 16].cpu().numpy(), tr.reward[:T].cpu().numpy(),
                        tr.done[:T].cpu().numpy(), self.config.ctrl_dt, self.config.render_track_body_id,
                        (self.kcfg.terrain_amp, self.kcfg.terrain_wavelength))
        rec.stats = stats
        if path is not None:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            rec.save_npz(path + ".npz")
            rec.save_html(path + ".html", title=f"kbot-joystick policy, iteration {self.iteration}: reward/step {stats['valid/reward_per_step']:.3f}")
        return rec

    def scalars(self) -> dict:
        """The scalars the reference's logger plots after each iteration (train.py:1783-1790): loss terms, reward, terminations."""
        m = self.metrics.cpu().tolist()
        names = ("loss", "policy_loss", "value_loss", "entropy", "clip_fraction", "approx_kl", "adv_mean", "adv_std", "action_mirror_loss", "value_mirror_loss")
        out = {f"train/{n}": v for n, v in zip(names, m)}
        done = self.traj.done
        st = torch.stack([self.traj.reward.mean(), (done < 0).float().mean(), (done > 0).float().mean(), self.traj.value.mean(), self.traj.logp.mean()]).cpu().tolist()   # one sync
        out["train/reward_per_step"], out["train/failures_per_step"], out["train/truncations_per_step"], out["train/value_mean"], out["train/action_std_logp"] = st
        if self.traj.comps is not None:
            for name, v in self.reward_components().items():
                out[f"reward/{name}"] = v
        for c in self._carriers:         # the results came back behind the kernels: the sync above is already past them
            out.update(self.episode_stats() if c is self.episodes else self._mode_stats(c, type(c), False))      # what <switch>() returns
        return out

    def export_actor(self, path: str):
        """convert.py's input: the actor's leaves, joint/command order and the flat carry size (host/export.py)."""
        from . import export
        c = self.kcfg
        export.export_actor(path, self.params.cpu().numpy(), self.H, c.depth, c.ctrl_dt, self.config.cutoff_frequency, c.min_std, c.max_std,
                            c.var_scale, list(self.model_blob.joint_bias), extra_obs=self.extra_obs)

    def deployed_actor(self, path: Optional[str] = None):
        """convert.py's init_fn / step_fn on the GPU (host/deploy.py DeployedActor: raw sensors + one flat carry per row -> action): of an
        `export_actor` archive at `path`, or - without a path - of this task's live parameters."""
        from . import deploy
        if path is not None:
            return deploy.DeployedActor.from_archive(path, self.device, robot=self.config.robot)
        return deploy.DeployedActor.from_params(self)

    def reward_components(self):
        """Mean of every unscaled reward term over the last rollout (train.py:1224-1256 order, spec/constants.REWARD_NAMES);
        needs `log_reward_components=True` in the config (kbj_rollout then also writes the [T][N][12] terms)."""
        if self.traj.comps is None:
            raise B.KbjError("reward_components() needs HumanoidWalkingTaskConfig.log_reward_components=True")
        return dict(zip(constants.REWARD_NAMES, self.traj.comps.mean(dim=(0, 1)).cpu().tolist()))

    @classmethod
    def launch(cls, config: HumanoidWalkingTaskConfig, num_iterations: int = 10, log_every: int = 1, run_dir: Optional[str] = None, quiet: bool = False):
        """train.py:1760: build the task and run the training loop (single process; bench.py / torchrun drive N GPUs).
        With `run_dir` (the reference's `humanoid_walking_task/run_N`): scalars go to `run_dir/logs` (CSV + TensorBoard event file),
        `run_dir/checkpoints/ckpt.bin` is rewritten every `save_every_n_seconds` (train.py:1788, convert.sh:4) and at the end, and a
        deterministic validation rollout runs every `valid_every_n_steps` iterations (train.py:1789)."""
        from .scalars import ScalarLogger
        task = cls(config)
        if getattr(config, "run_mode", "train") == "view":      # README.md:66-70 `python -m train run_mode=view`: no training, play the checkpointed policy
            # the mode exists to look at the TRAINED policy: without the run directory's checkpoint it would record the freshly initialised
            # one under a title that says "policy, iteration 0" - a plausible-looking, meaningless rollout. The reference's view mode loads the
            # run's checkpoint as well (README.md:66-70).
            ck = os.path.join(run_dir, "checkpoints", "ckpt.bin") if run_dir is not None else None
            if ck is None or not os.path.exists(ck):
                task.close()
                raise FileNotFoundError(f"run_mode=view plays the checkpointed policy: {ck or '<run_dir>/checkpoints/ckpt.bin'} does not exist "
                                        "(pass run_dir= of a finished or running training run; task.view() records the CURRENT parameters of a live task)")
            task.load_checkpoint(ck)
            out = os.path.join(run_dir if run_dir is not None else ".", "view", f"rollout_{task.iteration}")
            rec = task.view(out)
            if not quiet:
                print(f"run_mode=view: {out}.html / .npz ({rec.qpos.shape[0]} frames x {rec.qpos.shape[1]} envs, reward/step {rec.stats['valid/reward_per_step']:.4f})")
            return task
        logger, ckpt_path = None, None
        if run_dir is not None:
            logger = ScalarLogger(os.path.join(run_dir, "logs"))
            os.makedirs(os.path.join(run_dir, "checkpoints"), exist_ok=True)
            ckpt_path = os.path.join(run_dir, "checkpoints", "ckpt.bin")
        t0 = last_save = last_valid = time.time()
        stats = dict(iterations=0, validations=0, validation_seconds=0.0, checkpoints=0, checkpoint_seconds=0.0)
        for it in range(num_iterations):
            task.train_iteration()
            now = time.time()
            if it == 0:
                stats["first_iteration_seconds"] = now - t0      # one-time costs live here: code objects loaded at first launch, pinned staging buffers
            if (it + 1) % log_every == 0:
                sc = task.scalars()
                sc["perf/env_steps_per_s"] = task.env_steps_per_iteration() * (it + 1) / (now - t0)
                due = (config.valid_every_n_steps and (it + 1) % config.valid_every_n_steps == 0) or \
                      (config.valid_every_n_seconds and now - last_valid >= config.valid_every_n_seconds)
                if due:
                    tv = time.time()
                    sc.update(task.validate())
                    last_valid = now
                    stats["validations"] += 1; stats["validation_seconds"] += time.time() - tv
                if logger:
                    logger.log(task.iteration, sc)
                if not quiet:
                    print(f"iter {it + 1}: reward/step {sc['train/reward_per_step']:.4f} loss {sc['train/loss']:.4f} value_loss {sc['train/value_loss']:.4f} "
                          f"entropy {sc['train/entropy']:.3f} clipfrac {sc['train/clip_fraction']:.3f} | {sc['perf/env_steps_per_s']:.3e} env-steps/s")
            if ckpt_path and config.save_every_n_seconds and now - last_save >= config.save_every_n_seconds:
                tc = time.time()
                task.save_checkpoint(ckpt_path, background=True)     # snapshot now, container written under the next iterations
                last_save = now
                stats["checkpoints"] += 1; stats["checkpoint_seconds"] += time.time() - tc
            stats["iterations"] = it + 1
        # the loop as its user sees it: training iterations + scalar logging + validations + periodic checkpoints, up to here
        stats["loop_seconds"] = time.time() - t0
        stats["env_steps_per_s"] = task.env_steps_per_iteration() * stats["iterations"] / max(stats["loop_seconds"], 1e-9)
        # steady state: everything behind the first iteration (its logging included), as a benchmark's warm-up step is outside its timed region
        if stats["iterations"] > 1:
            stats["steady_env_steps_per_s"] = task.env_steps_per_iteration() * (stats["iterations"] - 1) / max(stats["loop_seconds"] - stats["first_iteration_seconds"], 1e-9)
        if ckpt_path:
            tc = time.time()
            task.save_checkpoint(ckpt_path)      # the final one in line: the file is complete when launch() returns
            stats["final_checkpoint_seconds"] = time.time() - tc
        if logger:
            logger.close()
        task.loop_stats = stats
        return task
