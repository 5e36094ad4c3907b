"""The task's configuration: `HumanoidWalkingTaskConfig` (the reference's field names and defaults, train.py:73-122, and its translation
into a kbj_config), the reference's launch block, and the learning-rate schedule. host/task.py re-exports all three."""
from __future__ import annotations

import dataclasses
import math
import os
from dataclasses import dataclass
from typing import Optional

from ..spec import layout as L
from . import wiring


def _env_flag(name: str, off=False):
    """A field whose default comes from the environment variable `name`, read when a config object is created: unset, "" and "0" give `off`;
    anything else gives True - or, where `off` is a string (KBJ_SOLVER, KBJ_ALLREDUCE), the variable's value."""
    def read():
        v = os.environ.get(name, "")
        return off if v in ("", "0") else v if isinstance(off, str) else True
    return dataclasses.field(default_factory=read)


@dataclass
class HumanoidWalkingTaskConfig:
    """Same field names and defaults as the reference config (train.py:73-122 + ksim.PPOConfig fields used in
    train.py:1761-1791). Defaults are the dataclass defaults of the reference, NOT the launch overrides."""
    # model (train.py:78-93)
    hidden_size: int = 128
    depth: int = 2
    var_scale: float = 0.5
    cutoff_frequency: float = 10.0
    # optimizer (train.py:95-114)
    learning_rate: float = 5e-4
    adam_weight_decay: float = 1e-5
    use_lr_decay: bool = False
    lr_decay_steps: int = 19_200_000
    lr_final_multiplier: float = 0.01
    actor_mirror_loss_scale: float = 1.0
    critic_mirror_loss_scale: float = 0.01
    # ksim.PPOConfig fields set by the launch block (train.py:1763-1781)
    num_envs: int = 4096
    batch_size: int = 512
    num_passes: int = 3
    rollout_length_seconds: float = 2.0
    entropy_coef: float = 0.004
    gamma: float = 0.94
    lam: float = 0.94
    dt: float = 0.004
    ctrl_dt: float = 0.02
    iterations: int = 8
    ls_iterations: int = 8
    action_latency_range: tuple = (0.003, 0.01)
    drop_action_prob: float = 0.05
    save_every_n_seconds: Optional[float] = 60
    valid_every_n_steps: Optional[int] = 100      # train.py:1789: deterministic (argmax) validation rollout every n iterations
    valid_every_n_seconds: Optional[float] = None # train.py:1790
    render_length_seconds: float = 10.0           # train.py:1785: length of a validation / view rollout
    max_values_per_plot: int = 50                 # train.py:1783 (plot thinning of the reference's logger; kept for name compatibility)
    render_track_body_id: int = 0                 # train.py:1784: the body the view's camera follows (0, the world, = the base)
    run_mode: str = "train"                       # README.md:66-70 `run_mode=view`: launch() plays the checkpointed policy instead of training (host/view.py)
    # the editable part of get_rewards() / get_commands() (train.py:1206-1256): overrides by reward name
    reward_scales: Optional[dict] = None          # e.g. {"feet_airtime": 2.0, "torque": 0.0}
    reward_params: Optional[dict] = None          # e.g. {"base_height": {"standard_height": 0.85}}
    command_ranges: Optional[dict] = None         # e.g. {"vx_range": (-0.5, 1.5)}; keys as UnifiedCommand's (train.py:1211-1217)
    # the editable part of get_terminations() (train.py:1258-1269): {"bad_z": {"unhealthy_z": 0.4}, "not_upright": {"max_radians": 0.785},
    # "episode_length": {"max_length_sec": 12}}; a threshold of -inf / +inf switches the built-in term off (a Python term may replace it)
    termination_params: Optional[dict] = None
    # build-specific
    robot: str = "kbot"                # train.py:1080 loads robot/kbot; BASELINE configs use kbot-headless
    seed: int = 0
    fixed_command: Optional[tuple] = None   # BASELINE configs[1]: flat-ground fixed joystick velocity command
    # a25: the in-tree samplers (UnifiedCommand train.py:725-752, 782-785; PlaneXYPositionReset train.py:834-836) derive their draws from the key
    # they are called with exactly as jax.random does (split = threefry over a counter, uniform = mantissa fill, bernoulli, randint:
    # kbj_config.command_mode = 2). The key each call RECEIVES is still this build's own (ksim's split tree is un-vendored), and no JAX is in the
    # image to produce fixtures: pinned by jax.random's public known answers only, UNVERIFIED against a live JAX. Off by default.
    jax_random_keys: bool = False
    terrain: str = "flat"                   # "flat" | "sine" (train.py:1081 loads the "sine" scene; BASELINE configs[4])
    terrain_amplitude: float = 0.05         # metres; the surface definition is this build's own
    terrain_wavelength: float = 2.0
    log_reward_components: bool = False     # keep the 12 unscaled reward terms of every rollout for logging (39 MB at 8192 x 100)
    # episode accounting on the device (kbj_episode_stats): episodic return, true episode length, termination causes and - with
    # log_reward_components - the per-episode sum of every reward term, carried per env across rollouts and through checkpoints;
    # read with task.episode_stats(), merged into scalars() / validate(). Off (the default; KBJ_EPISODE_STATS in the environment overrides
    # it, for A/B runs with tools/ab_bench.py): nothing is allocated, launched or logged.
    episode_stats: bool = _env_flag("KBJ_EPISODE_STATS")
    # command-tracking errors on the device (kbj_tracking_stats; host/tracking.py): the five tracking errors of every env-step in physical units
    # (m/s, rad/s, 1 - cos^2 of the half tilt angle, m, rad^2), split by the six command modes of UnifiedCommand and counted over the rows whose
    # command has been held for tracking_settle_seconds; merged into scalars() / validate() as track/<mode>/..., carried per env across rollouts
    # and through checkpoints. Off (the default; KBJ_TRACKING_STATS in the environment overrides it, for A/B runs with tools/ab_bench.py):
    # nothing is allocated, launched or logged. task.tracking_sweep() - the joystick response table - works with the switch off too.
    tracking_stats: bool = _env_flag("KBJ_TRACKING_STATS")
    tracking_settle_seconds: float = 0.5    # settle_steps = round(tracking_settle_seconds / ctrl_dt)
    # gait statistics on the device (kbj_gait_stats; host/gait.py): how the robot walks - swing and stance times, duty factor, step rate, double-support
    # and flight share, foot clearance, left/right asymmetry, hops, peak ground force and torque level, in seconds, metres and newtons, split by the
    # six command modes; merged into scalars() / validate() as gait/<mode>/..., carried per env across rollouts and through checkpoints. Off (the
    # default; KBJ_GAIT_STATS in the environment overrides it, for A/B runs with tools/ab_bench.py): nothing is allocated, launched or logged.
    # task.gait_sweep() - the gait table per command - works with the switch off too.
    gait_stats: bool = _env_flag("KBJ_GAIT_STATS")
    # actuator statistics on the device (kbj_actuator_stats; host/actuator.py): what the policy asks of the motors - per actuator torque against its
    # level, joint speed, mechanical power, joint stops, action rate - split by the six command modes; merged into scalars() / validate() as
    # act/<mode>/... (whole-body figures; the per-joint table comes from task.actuator_stats(per_joint=True)), carried per env across rollouts and
    # through checkpoints. Needs record_state (joint positions and speeds come from the state record). Off (the default; KBJ_ACTUATOR_STATS in the
    # environment overrides it): nothing is allocated, launched or logged. task.actuator_sweep() works with the switch off too.
    # The three levels are SETTINGS of this build, not figures of the reference (host/actuator.py actuator_levels): the share of
    # kbj_model.tau_limit that counts as "at the torque level", a speed limit in rad/s (None: none - the reference gives none; one float or 20)
    # and how far inside its range, in degrees, a joint counts as "at its stop".
    actuator_stats: bool = _env_flag("KBJ_ACTUATOR_STATS")
    actuator_torque_level: float = 0.9
    actuator_speed_limit: Optional[object] = None
    actuator_stop_margin_deg: float = 2.0
    # GAE boundary conventions (include/kbj.h kbj_gae). Both off by default - this build's choice: every termination ends the
    # return, V_T := V_{T-1} - and selectable, because SURVEY B.2 believes ksim bootstraps through the episode-length "success" termination:
    # bootstrap_on_truncation: at DONE = +1 (time-out, or a user term's +1) delta = r + gamma V(s_t) - V(s_t) instead of r - V(s_t);
    # bootstrap_tail_value: the last row bootstraps from the critic's value of observation row T (one more critic step per rollout) instead of
    # from V_{T-1}. KBJ_GAE_TRUNCATION / KBJ_GAE_TAIL in the environment override the defaults (A/B runs with tools/ab_bench.py).
    bootstrap_on_truncation: bool = _env_flag("KBJ_GAE_TRUNCATION")
    bootstrap_tail_value: bool = _env_flag("KBJ_GAE_TAIL")
    # bootstrap_terminal_value: what a bootstrapped truncation bootstraps FROM - the critic's value of the terminal observation (the state the episode
    # timed out in, before the reset; kbj_config.gae_terminal_value: the env step also writes that row, a sparse critic kernel values it, DESIGN.md
    # section 3) instead of V(s_t). It chooses among bootstraps, so it needs bootstrap_on_truncation and says so instead of switching it on.
    # Not with extra_critic_obs (user columns of a terminal row are not filled) nor record_state. KBJ_GAE_TERMINAL in the environment overrides the default.
    bootstrap_terminal_value: bool = _env_flag("KBJ_GAE_TERMINAL")
    # constraint solver of the physics step (kbj_config.solver_newton): "newton" (the default: the kernel this build is tuned and measured with) or
    # "cg", Polak-Ribiere CG on the M^-1-preconditioned gradient - SURVEY B.1 records it as ksim's default, and at the launch block's
    # iterations=8, ls_iterations=8 (train.py:1777-1778) it is a different dynamics, not a cosmetic switch (DESIGN.md section 3 "Solver").
    # KBJ_SOLVER in the environment overrides the default (A/B runs with tools/ab_bench.py).
    solver: str = _env_flag("KBJ_SOLVER", "newton")
    # keep qpos / qvel of every env-step (kbj_traj.qstate_d, 262 MB at 8192 x 100): the Python reward terms (extra_rewards) then see a
    # ksim-shaped `host.trajectory.Trajectory` - trajectory.qpos / .qvel / .xpos / .xquat / .obs[...] / .command["unified_command"] as the
    # reference's reward classes read them (train.py:138-506) - instead of the narrower TrajectoryView of the aux record
    record_state: bool = False
    # data-parallel exchange: "per_step" = all-reduce the gradient before every optimizer step (the
    # single-GPU-equivalent default); "per_pass" = north_star's "once per update" variant: accumulate the minibatch gradients of
    # a pass locally, ONE all-reduce and ONE optimizer step per pass (fewer, larger steps - a different algorithm). KBJ_ALLREDUCE
    # in the environment overrides the default.
    allreduce: str = _env_flag("KBJ_ALLREDUCE", "per_step")
    # per_step exchange only: all-reduce the actor's gradient slice on a second stream under the critic's tail of kbj_ppo_grad
    # (kbj_stream_wait_actor_grad), the critic's slice behind the call. Same result; pays only where the exchange is visible (N > 1)
    overlap_allreduce: bool = _env_flag("KBJ_OVERLAP_ALLREDUCE")
    # bit-reproducible update: fixed-order reductions instead of fp32 / fp64 atomics in the gradient (kbj_config.deterministic); the
    # reference's XLA program is deterministic by default, here it costs a few percent and is off unless asked for
    deterministic: bool = _env_flag("KBJ_DETERMINISTIC")
    # NOT the default, never the headline: the update's large backward GEMMs through the exact three-way bf16 operand split (kbj_config.gemm_bf16x3,
    # DESIGN.md section 10b): fp32 in, fp32 accumulate, fp32 out, every product exact up to 2^-23; faster and measured more accurate than the fp32 MFMA chain
    gemm_bf16x3: bool = _env_flag("KBJ_GEMM_X3")
    # user observations INTO the network rows (the reference's user appends terms to the lists run_actor / run_critic
    # concatenate, train.py:1351-1433): that many floats are appended behind the reference's 65 / 475 columns of every observation row, the input
    # projections and the parameter vector grow accordingly (kbj_config.extra_obs_*). Which terms fill them: HumanoidWalkingTask(
    # extra_observations={name: (term, "actor" | "critic" | "both")}); the widths must add up. 0..64 each.
    extra_actor_obs: int = 0
    extra_critic_obs: int = 0
    # data-parallel variant: normalise a minibatch's advantages with the mean / variance of the GLOBAL minibatch (all
    # ranks' minibatches of that step: three scalars all-reduced per step) instead of each rank's own. With it the averaged gradient equals the
    # single-process gradient over the union of the ranks' minibatches. Off by default (what ksim does across devices is not visible).
    global_advantage_stats: bool = _env_flag("KBJ_GLOBAL_ADV_STATS")
    # use_lr_decay with adam_weight_decay == 0 is train.py:1074-1075 AS WRITTEN: optax.chain(scale_by_adam(), scale_by_schedule(cosine)) has
    # no sign flip, i.e. gradient ASCENT. Served only with this explicit opt-in (recorded in the checkpoint's config member); without it
    # that combination is an error.
    reproduce_reference_lr_sign: bool = False

    def to_kbj(self, num_envs_local: int, env_id_offset: int = 0) -> L.Config:
        if self.batch_size <= 0 or num_envs_local % self.batch_size != 0:
            raise ValueError(f"batch_size {self.batch_size} must divide the per-GPU num_envs {num_envs_local}")
        # use_lr_decay with adam_weight_decay == 0 is train.py:1074-1075: optax.chain(scale_by_adam(), scale_by_schedule(cosine_schedule)).
        # AS WRITTEN that chain has no sign flip (optax.adam ends in scale_by_learning_rate = scale(-lr); scale_by_schedule does not), so
        # the parameters move ALONG the Adam direction: p += lr_t * m / (sqrt(v) + eps). It is served as written - kbj_adamw_step with
        # weight_decay 0 and the learning rate -cosine_decay_lr (update()) - behind reproduce_reference_lr_sign only; every rank says so at
        # construction and update() warns once, because it is gradient ascent.
        if self.use_lr_decay and self.adam_weight_decay == 0.0 and not self.reproduce_reference_lr_sign:
            raise ValueError("use_lr_decay with adam_weight_decay == 0 is train.py:1074-1075: optax.chain(scale_by_adam, scale_by_schedule) "
                             "has no sign flip, so the update ASCENDS the loss. Set reproduce_reference_lr_sign=True to run it as written, "
                             "or use a non-zero adam_weight_decay (the adamw branch, train.py:1076-1077)")
        T = int(round(self.rollout_length_seconds / self.ctrl_dt))
        kw = dict(num_envs=num_envs_local, env_id_offset=env_id_offset, rollout_len=T, substeps=int(round(self.ctrl_dt / self.dt)),
                  solver_iterations=self.iterations, ls_iterations=self.ls_iterations, solver_newton=int(self.solver == "newton"),
                  hidden_size=self.hidden_size, depth=self.depth,
                  batch_size=self.batch_size, num_passes=self.num_passes, dt=self.dt, ctrl_dt=self.ctrl_dt,
                  latency_lo=self.action_latency_range[0], latency_hi=self.action_latency_range[1],
                  drop_action_prob=self.drop_action_prob, var_scale=self.var_scale, entropy_coef=self.entropy_coef, gamma=self.gamma,
                  lam=self.lam, learning_rate=self.learning_rate, weight_decay=self.adam_weight_decay, switch_prob=self.ctrl_dt / 5,
                  actor_mirror_loss_scale=self.actor_mirror_loss_scale, critic_mirror_loss_scale=self.critic_mirror_loss_scale,
                  lpf_alpha=self.ctrl_dt / (self.ctrl_dt + 1.0 / (2.0 * math.pi * self.cutoff_frequency)), deterministic=int(bool(self.deterministic)),
                  extra_obs_actor=int(self.extra_actor_obs), extra_obs_critic=int(self.extra_critic_obs), gemm_bf16x3=int(bool(self.gemm_bf16x3)),
                  gae_bootstrap_truncation=int(bool(self.bootstrap_on_truncation)), gae_tail_value=int(bool(self.bootstrap_tail_value)),
                  gae_terminal_value=int(bool(self.bootstrap_terminal_value)))
        if self.bootstrap_terminal_value:
            if not self.bootstrap_on_truncation:
                raise ValueError("bootstrap_terminal_value chooses what a bootstrapped time-out bootstraps from (the terminal observation's value instead of "
                                 "V(s_t)): it needs bootstrap_on_truncation=True (KBJ_GAE_TRUNCATION=1) and does not switch it on by itself")
            if self.extra_critic_obs > 0:
                raise ValueError("bootstrap_terminal_value cannot be combined with extra_critic_obs > 0: the user columns of a terminal critic row are "
                                 "not filled (the terminal row is written inside the env step, before any observation term runs)")
            if self.record_state:
                raise ValueError("bootstrap_terminal_value cannot be combined with record_state: no env step kernel writes both the state record and "
                                 "the terminal critic rows")
        if self.actuator_stats and not self.record_state:
            raise ValueError("actuator_stats needs record_state=True: joint positions and speeds come from the per-step state record "
                             "(kbj_traj.qstate_d: 320 bytes per env-step, 262 MB at 8192 envs x 100 steps)")
        if not (0 <= self.extra_actor_obs <= L.MAX_EXTRA_OBS and 0 <= self.extra_critic_obs <= L.MAX_EXTRA_OBS):
            raise ValueError(f"extra_actor_obs / extra_critic_obs must be in 0..{L.MAX_EXTRA_OBS}")
        if self.solver not in ("newton", "cg"):
            raise ValueError(f"unknown solver {self.solver!r} (newton | cg)")
        if self.allreduce not in ("per_step", "per_pass"):
            raise ValueError(f"unknown allreduce mode {self.allreduce!r} (per_step | per_pass)")
        if self.terrain not in ("flat", "sine"):
            raise ValueError(f"unknown terrain {self.terrain!r} (flat | sine)")
        if self.terrain == "sine":
            kw.update(terrain_amp=self.terrain_amplitude, terrain_wavelength=self.terrain_wavelength)
        if self.jax_random_keys:
            kw.update(command_mode=2)           # (a fixed command below overrides the sampler, not the reset's key handling... which command_mode 1 switches off too)
        if self.fixed_command is not None:
            if self.jax_random_keys:
                raise ValueError("jax_random_keys selects the UnifiedCommand SAMPLER with jax.random's key handling; it cannot be combined with fixed_command")
            cmd = list(self.fixed_command) + [0.0] * (L.NCMD - len(self.fixed_command))
            kw.update(command_mode=1, fixed_command=cmd)
        for k, (lo, hi) in (self.command_ranges or {}).items():
            if k not in ("vx_range", "vy_range", "wz_range", "bh_range", "rx_range", "ry_range"):
                raise KeyError(f"unknown command range {k!r}")
            kw[k[:2] + "_lo"], kw[k[:2] + "_hi"] = float(lo), float(hi)
        for name, kv in (self.termination_params or {}).items():
            for k, v in kv.items():
                v = float(v)
                if (name, k) == ("bad_z", "unhealthy_z"):
                    kw["unhealthy_z"] = max(v, -3.0e38)
                elif (name, k) == ("not_upright", "max_radians"):
                    kw["max_tilt_rad"] = min(v, math.pi)
                elif (name, k) == ("episode_length", "max_length_sec"):
                    # round like T and substeps: 2.3 / 0.02 is 115, not 114; +inf (the documented "off") has no integer to round to
                    kw["max_episode_steps"] = 2 ** 30 if math.isinf(v) and v > 0 else int(min(round(v / self.ctrl_dt), 2 ** 30))
                else:
                    raise KeyError(f"unknown termination parameter {name}.{k} (bad_z.unhealthy_z | not_upright.max_radians | episode_length.max_length_sec)")
        kcfg = L.default_config(**kw)
        wiring.apply_reward_overrides(kcfg, self.reward_scales, self.reward_params)
        return kcfg



def cosine_decay_lr(config: HumanoidWalkingTaskConfig, count: int) -> float:
    """optax.cosine_decay_schedule(init_value, decay_steps, alpha) at optimizer-update count `count` (train.py:1068-1072)."""
    frac = min(max(count, 0), config.lr_decay_steps) / config.lr_decay_steps
    cosine = 0.5 * (1.0 + math.cos(math.pi * frac))
    return config.learning_rate * ((1.0 - config.lr_final_multiplier) * cosine + config.lr_final_multiplier)


def launch_config(**overrides) -> HumanoidWalkingTaskConfig:
    """The reference's launch block (train.py:1761-1791)."""
    kw = dict(num_envs=4096, batch_size=512, num_passes=3, rollout_length_seconds=2.0, entropy_coef=0.004, learning_rate=5e-4, gamma=0.94,
              lam=0.94, actor_mirror_loss_scale=0.0, critic_mirror_loss_scale=0.0, hidden_size=256, dt=0.004, ctrl_dt=0.02, iterations=8,
              ls_iterations=8, action_latency_range=(0.003, 0.01), drop_action_prob=0.05, render_track_body_id=0, render_length_seconds=10,
              max_values_per_plot=50, save_every_n_seconds=60, valid_every_n_steps=100, valid_every_n_seconds=None)
    kw.update(overrides)
    return HumanoidWalkingTaskConfig(**kw)
