/* kbj_model.h — shared DATA FORMATS of the K-Bot joystick hot path (no algorithms).
 *
 * Everything here is a plain-C description of bytes that cross the C ABI in kbj.h:
 *   - kbj_model   : the compiled robot ("model blob"), replaces mujoco.MjModel for this path
 *                   (reference: train.py:1079-1089 get_mujoco_model / get_mujoco_model_metadata,
 *                    robot/<name>/robot.mjcf, robot/<name>/metadata.json)
 *   - kbj_config  : run-time configuration (reference: train.py:73-122 config dataclass,
 *                   train.py:1759-1792 launch values, train.py:1091-1276 task wiring constants)
 *   - per-env parameter / state records and the trajectory record layouts (float offsets)
 *
 * The kbot topology is fixed (24 bodies, 1 free + 20 hinge joints, 4 foot capsules); the HIP
 * kernels are specialised on it and kbj_create() rejects blobs with a different topology.
 */
#ifndef KBJ_MODEL_H
#define KBJ_MODEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KBJ_MAGIC   0x4D4A424Bu /* "KBJM" little endian */
#define KBJ_VERSION 3u

#define KBJ_NBODY 24 /* incl. world (0) */
#define KBJ_NQ    27
#define KBJ_NV    26
#define KBJ_NU    20
#define KBJ_NCAP  4  /* collision capsules (2 per foot) */
#define KBJ_NCON  8  /* capsule-plane: one contact per capsule end */
#define KBJ_NCMD  16
#define KBJ_NREW  12

/* observation vector sizes (train.py:1281-1312) and their row strides in HBM (16-B aligned rows) */
#define KBJ_NOBS_ACTOR   65
#define KBJ_NOBS_CRITIC  475
#define KBJ_LD_ACTOR     68
#define KBJ_MAX_DEPTH    4   /* LSTM layers per net the library's workspaces are laid out for */
#define KBJ_LD_CRITIC    476
/* User observations INTO the network rows (kbj_config.extra_obs_actor / extra_obs_critic, the f3 row of SURVEY.md section 8): the reference's
 * user appends terms to the lists run_actor / run_critic concatenate (train.py:1351-1433); here up to KBJ_MAX_EXTRA_OBS floats are appended
 * BEHIND the reference's 65 / 475 (every KBJ_OBS_* offset stays put). Row widths and strides of a context:
 *   nobs = KBJ_NOBS_x + extra_obs_x,  ld = KBJ_LD_OF(nobs)  (rows stay 16-byte aligned; the pad columns are zero)
 * The env kernels write the reference's columns and zero [KBJ_NOBS_x, ld); the host writes its terms' outputs behind them. */
#define KBJ_MAX_EXTRA_OBS 64
#define KBJ_LD_OF(nobs)  (((nobs) + 3) & ~3)

/* Offsets of the pieces of a packed observation row, in the order run_actor / run_critic concatenate them (train.py:1367-1374,
 * 1410-1430); the first 65 entries are common to both rows, the critic's privileged pieces follow. Divisors as train.py:1336, 1427.
 * tests/test_ref_constants.py derives this table from the reference's source text (ast) and asserts it. */
enum {
  KBJ_OBS_JPOS     = 0,    /* [20] normalize_joint_pos(joint position) */
  KBJ_OBS_JVEL     = 20,   /* [20] joint velocity / KBJ_OBS_JVEL_DIV */
  KBJ_OBS_PG       = 40,   /* [5]  roll, pitch, unit projected gravity */
  KBJ_OBS_GYRO     = 45,   /* [3]  */
  KBJ_OBS_ZEROCMD  = 48,   /* [1]  |cmd[0:3]| < 1e-3 */
  KBJ_OBS_CMD      = 49,   /* [16] unified command */
  KBJ_OBS_TOUCH    = 65,   /* [2]  left, right foot touch (critic only from here) */
  KBJ_OBS_FEETPOS  = 67,   /* [6]  */
  KBJ_OBS_BASEPOS  = 73,   /* [3]  */
  KBJ_OBS_BASEQUAT = 76,   /* [4]  */
  KBJ_OBS_CINERT   = 80,   /* [23][10] */
  KBJ_OBS_CVEL     = 310,  /* [23][6]  */
  KBJ_OBS_LINVEL   = 448,  /* [3]  */
  KBJ_OBS_ANGVEL   = 451,  /* [3]  */
  KBJ_OBS_ACTFRC   = 454,  /* [20] actuator force / KBJ_OBS_ACTFRC_DIV */
  KBJ_OBS_HEIGHT   = 474   /* [1]  */
};
#define KBJ_OBS_JVEL_DIV   10.0f
#define KBJ_OBS_ACTFRC_DIV 4.0f

typedef struct kbj_model {
  uint32_t magic, version;
  int32_t  nbody, nq, nv, nu, ncap, reserved0;
  int32_t  body_parent[KBJ_NBODY];
  int32_t  body_dofadr[KBJ_NBODY]; /* first dof of the body's joint, -1 if none */
  int32_t  body_dofnum[KBJ_NBODY]; /* 0 (welded), 1 (hinge), 6 (free) */
  int32_t  dof_body[KBJ_NV];
  int32_t  dof_parent[KBJ_NV];     /* previous dof up the tree, -1 at the root */
  int32_t  cap_body[KBJ_NCAP];
  int32_t  base_body, torso_body, lfoot_body, rfoot_body, imu_body, reserved1[3];
  float    body_pos[KBJ_NBODY][3];
  float    body_quat[KBJ_NBODY][4];   /* w,x,y,z relative to parent */
  float    body_ipos[KBJ_NBODY][3];
  float    body_mass[KBJ_NBODY];
  float    body_inertia[KBJ_NBODY][3]; /* diagonal, inertial frame == body frame for this robot */
  float    jnt_axis[KBJ_NBODY][3];     /* hinge axis in the body frame (bodies with dofnum==1) */
  float    qpos0[KBJ_NQ];
  float    reserved2;
  float    dof_armature[KBJ_NV];
  float    dof_frictionloss[KBJ_NV];
  float    dof_invweight0[KBJ_NV];
  float    dof_range[KBJ_NV][2];       /* joint limits by dof (first 6 unused) */
  float    act_range[KBJ_NU][2];       /* motor ctrlrange == joint actuatorfrcrange */
  float    body_invweight0[KBJ_NBODY][2];
  float    cap_pos[KBJ_NCAP][3];       /* capsule centre in body frame */
  float    cap_axis[KBJ_NCAP][3];      /* unit axis in body frame */
  float    cap_halflen[KBJ_NCAP];
  float    cap_radius[KBJ_NCAP];
  float    site_pos[2][3];             /* foot touch boxes (left, right), body frame, axis aligned */
  float    site_size[2][3];
  float    imu_quat[4];                /* imu_site orientation in the imu body */
  float    contact_mu;
  float    contact_solref[2];
  float    contact_solimp[5];
  float    limit_solref[2];
  float    limit_solimp[5];
  float    fric_solref[2];
  float    fric_solimp[5];
  float    gravity[3];
  float    kp[KBJ_NU], kd[KBJ_NU], tau_limit[KBJ_NU]; /* metadata.json per-joint gains */
  float    joint_bias[KBJ_NU];  /* train.py:24-45  */
  float    joint_lo[KBJ_NU];    /* train.py:47-68  */
  float    joint_hi[KBJ_NU];
  float    total_mass;
  float    meaninertia;
  float    reserved3[2];
} kbj_model;

/* Run-time configuration. Defaults (kbj_config_default in the host layer) follow the launch block
 * train.py:1759-1792 and the task wiring train.py:1091-1276; ksim-internal defaults that are not
 * visible in the reference tree are our own documented choices (DESIGN.md "Spec decisions"). */
typedef struct kbj_config {
  int32_t num_envs;          /* envs on THIS gpu */
  int32_t env_id_offset;     /* global id of local env 0 (rank * num_envs) -> RNG streams independent of gpu count */
  int32_t rollout_len;       /* T control steps per rollout (100 = 2.0 s / 0.02 s) */
  int32_t substeps;          /* ctrl_dt / dt = 5 */
  int32_t solver_iterations; /* 8 */
  int32_t ls_iterations;     /* 8 */
  int32_t hidden_size;       /* 256 launch / 128 dataclass default */
  int32_t depth;             /* LSTM layers per net, 1..KBJ_MAX_DEPTH (train.py:82-85: 2) */
  int32_t batch_size;        /* envs per minibatch */
  int32_t num_passes;
  int32_t command_mode;      /* 0 = UnifiedCommand sampler (train.py:710-785); 1 = fixed command; 2 = the sampler (and PlaneXYPositionReset,
                                train.py:834-836) with jax.random's own key handling below the call key: split / uniform / bernoulli / randint as jax
                                0.6.0 derives them from a threefry key (csrc/kbj_env_core.h "jax.random key handling"; UNVERIFIED against a live JAX) */
  int32_t enable_randomizers;
  int32_t enable_pushes;
  int32_t enable_noise;
  int32_t max_episode_steps; /* 12 s / 0.02 s = 600 */
  int32_t solver_newton;     /* constraint solver of the physics step, both served by their own HIP kernels. 1 (default) = Newton direction with the exact
                              * Hessian; 0 = Polak-Ribiere CG on the M^-1-preconditioned gradient: search = -Mgrad + max(0, grad.(Mgrad - Mgrad_old) /
                              * (grad_old.Mgrad_old)) search, the first iteration of a solve steepest descent. Warm start, exit tests and line search
                              * are shared. At the launch block's iterations=8, ls_iterations=8 (train.py:1777-1778) CG stops at the cap where
                              * Newton has converged: a different dynamics. Any other value is refused (kbj_check_config) */
  int32_t deterministic;     /* 1 = the PPO update reduces in a fixed order (split-K slabs, per-block partials) instead of with fp32 / fp64 atomics:
                                two updates from the same state give bit-identical parameters, as the reference's XLA program does; default 0 */
  int32_t extra_obs_actor;   /* floats the host appends to every actor / critic observation row (0..KBJ_MAX_EXTRA_OBS, default 0): the input */
  int32_t extra_obs_critic;  /* projections are [H][65 + extra] / [H][475 + extra], the parameter vector grows accordingly */
  int32_t gemm_bf16x3;       /* 1 = the PPO update's large backward GEMMs (input gradients, weight-gradient pairs) run on the bf16 matrix cores through an
                                EXACT three-way split of their fp32 operands (6 bf16 products per fp32 product, fp32 accumulation): measured more
                                accurate than the fp32-MFMA chain and faster. Default 0: the plain fp32-MFMA kernels, which is
                                what every headline number of this library is measured with. Ignored in deterministic mode. */
  int32_t gae_bootstrap_truncation; /* kbj_gae at a TRUNCATION (KBJ_AUX_DONE > 0: the episode-length "success" termination, or a user term's +1):
                                0 (default) = a terminal state like a failure, delta = r - V(s_t); 1 = bootstrap through it with V(s_t) standing
                                in for the unrecorded terminal observation, delta = r + gamma V(s_t) - V(s_t). The advantage chain is cut either way. */
  int32_t gae_tail_value;    /* kbj_gae at the END of a rollout: 0 (default) = V_T := V_{T-1}; 1 = V_T = kbj_traj.value_tail_d, the critic's value of
                                observation row T from the post-rollout carries (kbj_rollout / kbj_critic_value write it). 0 or 1, kbj.h kbj_gae */
  float dt;                 /* 0.004 */
  float ctrl_dt;             /* 0.02  */
  float solver_tolerance;    /* 1e-8 */
  float latency_lo, latency_hi; /* seconds (0.003, 0.01) */
  float drop_action_prob;    /* 0.05 */
  float fixed_command[KBJ_NCMD];
  /* command ranges train.py:1211-1221 */
  float vx_lo, vx_hi, vy_lo, vy_hi, wz_lo, wz_hi, bh_lo, bh_hi, rx_lo, rx_hi, ry_lo, ry_hi;
  float switch_prob;         /* ctrl_dt / 5 */
  /* resets train.py:1146-1153 */
  float reset_joint_pos_scale, reset_joint_vel_scale, reset_base_vel_xy_scale, reset_xy_range;
  /* terminations train.py:1258-1269 */
  float unhealthy_z, max_tilt_rad;
  /* actuator randomisation train.py:1097-1105 */
  float kp_scale, kd_scale, torque_limit_scale_low, action_bias_scale, torque_bias_scale;
  /* physics randomisers train.py:1107-1132 */
  float fricloss_scale_lo, fricloss_scale_hi, armature_scale_lo, armature_scale_hi;
  float floor_friction_lo, floor_friction_hi, com_jitter, inertia_scale;
  float cap_radius_scale, cap_length_scale, cap_jitter[3];
  /* push event train.py:1134-1144 */
  float push_max_force, push_max_torque, push_dur_lo, push_dur_hi, push_int_lo, push_int_hi;
  /* observation noise train.py:1156-1204 */
  float jpos_bias_range, jpos_noise, jvel_noise, gyro_noise_std, pg_noise_std, pg_lag_lo, pg_lag_hi, pg_bias;
  /* actor head train.py:1320-1326 */
  float min_std, max_std, var_scale, lpf_alpha;
  /* ppo (ksim defaults restated) */
  float gamma, lam, clip_param, value_loss_coef, entropy_coef, log_ratio_clip, max_grad_norm;
  float learning_rate, adam_b1, adam_b2, adam_eps, weight_decay, adv_eps;
  float value_clip;          /* clipped value loss range */
  float actor_mirror_loss_scale;  /* train.py:115-122 (dataclass defaults 1.0 / 0.01; launch config 0.0 / 0.0, train.py:1771-1772) */
  float critic_mirror_loss_scale;
  /* terrain ("sine" scene, train.py:1081; the surface is this build's own definition):
   * z = terrain_amp * sin(2 pi x / terrain_wavelength) * sin(2 pi y / terrain_wavelength); terrain_amp = 0 is the plane z = 0 */
  float terrain_amp, terrain_wavelength;
  int32_t gae_terminal_value; /* kbj_gae at a TRUNCATION once gae_bootstrap_truncation = 1: 0 (default) = bootstrap from V(s_t); 1 = from the critic's value of
                                the TERMINAL observation - the state the episode ended in, before the reset - which kbj_rollout / kbj_env_step_terminal +
                                kbj_critic_terminal_value record into the buffer of kbj_set_terminal_values. 1 with gae_bootstrap_truncation = 0 is refused.
                                (One word of the former reserved_f[4]: the struct's size and every other offset are unchanged.) */
  float reserved_f[3];
  /* reward stack (train.py:1224-1256): the scale of every term in KBJ_REW_* order, then the constructor arguments the reference
   * passes to its reward classes (error scales, heights, grace period, touchdown penalty). User-editable like the reference's
   * get_rewards(); a scale of 0 switches a term off. */
  float reward_scale[12];
  float rew_linvel_err, rew_angvel_err, rew_rollpitch_err, rew_rollpitch_err_zero;   /* train.py:1227-1229 */
  float rew_height_err, rew_standard_height, rew_foot_origin_height;                 /* train.py:1230-1239 */
  float rew_armpos_err, rew_grace_period, rew_touchdown_penalty;                     /* train.py:1240-1244 */
  float rew_feetorient_err, rew_comdist_err, rew_baseaccel_err, rew_torque_err;      /* train.py:1245-1255 */
  float reserved_r[2];
} kbj_config;

/* ---- per-env randomised model parameters ("EP" record, floats, one contiguous row per env) ---- */
enum {
  KBJ_EP_IPOS     = 0,    /* [24][3] */
  KBJ_EP_MASS     = 72,   /* [24]    */
  KBJ_EP_INERTIA  = 96,   /* [24][3] */
  KBJ_EP_ARMATURE = 168,  /* [26]    */
  KBJ_EP_FRICLOSS = 194,  /* [26]    */
  KBJ_EP_CAP_POS  = 220,  /* [4][3]  */
  KBJ_EP_CAP_HALF = 232,  /* [4]     */
  KBJ_EP_CAP_RAD  = 236,  /* [4]     */
  KBJ_EP_KP       = 240,  /* [20]    */
  KBJ_EP_KD       = 260,
  KBJ_EP_TAULIM   = 280,
  KBJ_EP_ACTBIAS  = 300,
  KBJ_EP_JPBIAS   = 320,  /* [20] biased joint position observation offset */
  KBJ_EP_PGBIAS   = 340,  /* [3]  projected-gravity bias */
  KBJ_EP_PGLAG    = 343,
  KBJ_EP_LATENCY  = 344,  /* action latency in substeps (integer valued) */
  KBJ_EP_MU       = 345,  /* contact friction */
  KBJ_EP_SIZE     = 352
};

/* ---- per-env persistent state ("ES" record, floats; uint32 fields are bit-cast) ---- */
enum {
  KBJ_ES_QPOS     = 0,    /* [27] */
  KBJ_ES_QVEL     = 28,   /* [26] */
  KBJ_ES_WARM     = 54,   /* [26] qacc warm start */
  KBJ_ES_ACT_PREV = 80,   /* [20] action applied during the previous control step */
  KBJ_ES_CMD      = 100,  /* [16] */
  KBJ_ES_PUSH     = 116,  /* [6] force(3) torque(3) world frame */
  KBJ_ES_PUSH_REM = 122,  /* control steps of push remaining (a float holding a whole number; the step kernel counts it down once per control step) */
  KBJ_ES_PUSH_NXT = 123,  /* control steps until the built-in event draws its next push (not counted down while PUSH_REM > 0); KBJ_PUSH_NEVER holds it off */
  KBJ_ES_TIME     = 124,  /* control steps since episode start */
  KBJ_ES_PGLAG    = 125,  /* [3] lagged projected gravity */
  KBJ_ES_EPISODE  = 128,  /* uint32 episode counter (RNG stream) */
  KBJ_ES_STEP     = 129,  /* uint32 global control-step counter  */
  KBJ_ES_SIZE     = 136
};

/* ---- reward carry per env (StatefulReward carries, train.py:135-136,175-178) ---- */
enum {
  KBJ_RC_TSINGLE  = 0,   /* time since single contact, initial 0 */
  KBJ_RC_AIRTIME  = 1,   /* [2] initial 0 */
  KBJ_RC_CONTACT  = 3,   /* [2] previous contact flags, initial 1 (True) */
  KBJ_RC_SIZE     = 8
};

/* ---- per env-step "aux" record: everything the reward stack reads (train.py:125-506) ---- */
enum {
  KBJ_AUX_QVEL    = 0,   /* [6] base qvel after the step */
  KBJ_AUX_BQUAT   = 6,   /* [4] xquat[base] */
  KBJ_AUX_BASEZ   = 10,
  KBJ_AUX_LFZ     = 11,
  KBJ_AUX_RFZ     = 12,
  KBJ_AUX_LFQUAT  = 13,  /* [4] */
  KBJ_AUX_RFQUAT  = 17,  /* [4] */
  KBJ_AUX_ARMQ    = 21,  /* [10] qpos of the arm joints */
  KBJ_AUX_CTRL    = 31,  /* [20] torque command of the last substep */
  KBJ_AUX_TOUCH   = 51,  /* [2] observation (pre-step) */
  KBJ_AUX_COMDIST = 53,  /* observation (pre-step) */
  KBJ_AUX_CMD     = 54,  /* [16] command the policy saw */
  KBJ_AUX_DONE    = 70,  /* -1 failure, 0 running, +1 episode-length truncation */
  KBJ_AUX_SIZE    = 72
};

/* ---- optional per env-step state record (kbj_traj.qstate_d / kbj_env_record_state): the generalised state a ksim Trajectory step holds
 * (`trajectory.qpos`, `.qvel`: train.py:262, 286, 301, 488) plus the positions the step's LAST forward pass ran on, from which the body poses
 * of that pass (`trajectory.xpos`, `.xquat`: train.py:276, 317, 378-383, 419-444 - as in mj_step, the derived quantities a step leaves behind
 * are those of its last substep's kinematics, one integration behind qpos) follow by forward kinematics over the model blob's tree ---- */
enum {
  KBJ_QSTATE_QPOS     = 0,    /* [27] qpos after the step (before any reset) */
  KBJ_QSTATE_QVEL     = 27,   /* [26] qvel after the step */
  KBJ_QSTATE_QPOS_KIN = 53,   /* [27] qpos the last substep's forward pass (xpos, xquat, sensors, contacts) was computed from */
  KBJ_QSTATE_SIZE     = 80
};

/* ---- episode accounting (kbj_episode_stats) ----
 * Per-env accumulator row ("EACC" record, fp32, owned by the caller on the device like kbj_carry): what the env's RUNNING episode has
 * collected so far; carried from one rollout to the next, zeroed when the episode ends. */
enum {
  KBJ_EACC_RETURN = 0,   /* sum of reward since the episode started */
  KBJ_EACC_LENGTH = 1,   /* control steps since the episode started (integer valued) */
  KBJ_EACC_TERM   = 2,   /* [12] sums of the unscaled reward terms, KBJ_REW_* order (stay 0 without kbj_traj.reward_comps_d) */
  KBJ_EACC_SIZE   = 16   /* 64-byte rows; the two spare floats are left as they are */
};
/* One call's result ("EPST" record, doubles): statistics of the episodes that FINISHED inside the trajectory. The cause slots double as
 * the cause codes. With no finished episode RETURN_MIN = +inf, RETURN_MAX = -inf, LENGTH_MAX = 0; spare slots are 0. */
enum {
  KBJ_EPST_EPISODES        = 0,   /* episodes that finished in this trajectory = the sum of the next three */
  KBJ_EPST_FAIL_HEIGHT     = 1,   /* done < 0 and BASEZ - fminf(LFZ, RFZ) < unhealthy_z (the env kernel's own fp32 expression) */
  KBJ_EPST_FAIL_OTHER      = 2,   /* done < 0 otherwise (tilt only, or a user Termination term's -1) */
  KBJ_EPST_TRUNCATED       = 3,   /* done > 0 (episode length, or a user term's +1) */
  KBJ_EPST_RETURN_SUM      = 4,   /* over the finished episodes: sum of the fp32 episodic return, */
  KBJ_EPST_RETURN_SUMSQ    = 5,   /* of its square (taken in double), */
  KBJ_EPST_RETURN_MIN      = 6,   /* its minimum */
  KBJ_EPST_RETURN_MAX      = 7,   /* and maximum */
  KBJ_EPST_LENGTH_SUM      = 8,   /* sum of the episode lengths (control steps), */
  KBJ_EPST_LENGTH_MAX      = 9,   /* the longest, */
  KBJ_EPST_FAIL_LENGTH_SUM = 10,  /* the sum over the done < 0 episodes only */
  KBJ_EPST_TERM_SUM        = 12,  /* [12] sum over the finished episodes of the episodic reward-term sums, KBJ_REW_* order */
  KBJ_EPST_SIZE            = 32
};

/* ---- command-tracking errors (kbj_tracking_stats) ----
 * Mode of a row, from its command alone (exact != 0.0f tests; numbering = the switch list of train.py:752-762). */
enum {
  KBJ_CMODE_FORWARD    = 0,   /* only cmd[0] non-zero */
  KBJ_CMODE_SIDEWAYS   = 1,   /* only cmd[1] non-zero */
  KBJ_CMODE_ROTATE     = 2,   /* only cmd[2] non-zero */
  KBJ_CMODE_OMNI       = 3,   /* moving with a pose (any of cmd[3:16] non-zero), or more than one of cmd[0:3] non-zero */
  KBJ_CMODE_STAND_BEND = 4,   /* cmd[0:3] zero, a pose */
  KBJ_CMODE_STAND      = 5,   /* all zero */
  KBJ_CMODE_COUNT      = 6
};
#define KBJ_NTERR 5 /* tracking errors per row */
/* One row of the optional per-row output ("TERR" record, fp32): the five errors in physical units, then three integer-valued floats. */
enum {
  KBJ_TERR_LIN     = 0,   /* |qvel_xy - R_yaw(base) cmd[0:2]|, m/s (train.py:274-290) */
  KBJ_TERR_YAW     = 1,   /* |qvel[5] - cmd[2]|, rad/s (train.py:301-305) */
  KBJ_TERR_TILT    = 2,   /* 1 - <q(roll, pitch, 0), q(cmd[4], cmd[5], 0)>^2 (train.py:316-330) */
  KBJ_TERR_HEIGHT  = 3,   /* |BASEZ - min(LFZ, RFZ) + foot_origin_height - (cmd[3] + standard_height)|, m (train.py:377-386) */
  KBJ_TERR_ARM     = 4,   /* sum_j (ARMQ[j] - cmd[6 + j] - joint_bias[10 + j])^2, rad^2 (train.py:261-264) */
  KBJ_TERR_MODE    = 5,   /* KBJ_CMODE_* of the row */
  KBJ_TERR_SETTLED = 6,   /* 1 when the row is counted: since >= settle_steps */
  KBJ_TERR_SINCE   = 7,   /* rows since the command last changed or the episode started, as used for this row */
  KBJ_TERR_SIZE    = 8
};
/* Per-env carry row ("TACC" record, fp32, owned by the caller on the device like the EACC rows; zeroed once). */
enum {
  KBJ_TACC_CMD     = 0,   /* [16] the command of the env's previous row */
  KBJ_TACC_SINCE   = 16,  /* rows since the command last changed or the episode started (integer valued, stops growing at 2^24) */
  KBJ_TACC_RUNNING = 17,  /* 1 when a previous row exists and did not end its episode */
  KBJ_TACC_SIZE    = 20   /* 80-byte rows; the two spare floats are left as they are */
};
/* One call's result ("TRK" record, doubles): KBJ_CMODE_COUNT mode blocks of KBJ_TRK_MODE_STRIDE slots (mode m's slot s at
 * m * KBJ_TRK_MODE_STRIDE + s), then the two counters; every other slot is 0. */
enum {
  KBJ_TRK_ROWS        = 0,    /* rows of the mode */
  KBJ_TRK_SETTLED     = 1,    /* of them settled; the next three groups are over the settled rows only */
  KBJ_TRK_SUM         = 2,    /* [5] sum of the fp32 error, KBJ_TERR_* order, */
  KBJ_TRK_SUMSQ       = 7,    /* [5] of its square (taken in double), */
  KBJ_TRK_MAX         = 12,   /* [5] its maximum (0 without settled rows: the errors are non-negative) */
  KBJ_TRK_MODE_STRIDE = 20,
  KBJ_TRK_CHANGES     = 120,  /* rows whose command differs from the previous row's inside a running episode */
  KBJ_TRK_EPISODES    = 121,  /* rows that start an episode (no previous row, or the previous row ended its episode) */
  KBJ_TRK_SIZE        = 128
};

/* ---- gait statistics (kbj_gait_stats) ----
 * Per-env carry row ("GACC" record, fp32, owned by the caller on the device like the TACC rows; zeroed once). Foot f (0 left, 1 right) keeps
 * its five floats at KBJ_GACC_FOOT_STRIDE * f. */
enum {
  KBJ_GACC_CON         = 0,   /* 1 when the foot was in contact on the env's previous row */
  KBJ_GACC_RUN         = 1,   /* rows the current phase (stance or swing) has lasted, the previous row included (integer valued, stops growing at 2^24) */
  KBJ_GACC_VALID       = 2,   /* 1 when the current phase began inside the episode: its duration and clearance count when it ends */
  KBJ_GACC_ZST         = 3,   /* the foot height on its last contact row (on the episode's first row while it has had none) */
  KBJ_GACC_PEAK        = 4,   /* the largest rise over ZST in the current swing */
  KBJ_GACC_FOOT_STRIDE = 6,   /* one spare float per foot, left as it is */
  KBJ_GACC_RUNNING     = 12,  /* 1 when a previous row exists and did not end its episode */
  KBJ_GACC_LAST_TD     = 13,  /* the foot of the episode's last touchdown, -1 before the first */
  KBJ_GACC_SIZE        = 16   /* 64-byte rows; the two spare floats at the end are left as they are */
};
/* One call's result ("GAIT" record, doubles): KBJ_CMODE_COUNT mode blocks of KBJ_GAIT_MODE_STRIDE slots (mode m's slot s at
 * m * KBJ_GAIT_MODE_STRIDE + s): seven row slots, then one block of KBJ_GAIT_FOOT_STRIDE foot slots per foot at KBJ_GAIT_FOOT +
 * KBJ_GAIT_FOOT_STRIDE * f; then the episode counter. Every other slot is 0. Durations are in rows. */
enum {
  KBJ_GAIT_ROWS         = 0,    /* rows of the mode */
  KBJ_GAIT_DOUBLE       = 1,    /* of them with both feet in contact, */
  KBJ_GAIT_SINGLE       = 2,    /* with one, */
  KBJ_GAIT_FLIGHT       = 3,    /* with none */
  KBJ_GAIT_REPEATS      = 4,    /* touchdowns of the foot that had the episode's previous touchdown too (a hop) */
  KBJ_GAIT_TORQUE_SQ    = 5,    /* sum over the rows of sum_u ctrl[u]^2 (taken in double) */
  KBJ_GAIT_TORQUE_MAX   = 6,    /* largest |ctrl[u]| */
  KBJ_GAIT_FOOT         = 8,    /* the first foot block */
  KBJ_GAIT_FOOT_STRIDE  = 16,
  KBJ_GAIT_MODE_STRIDE  = 40,
  KBJ_GAIT_EPISODES     = 240,  /* rows that start an episode (no previous row, or the previous row ended its episode) */
  KBJ_GAIT_SIZE         = 256
};
/* Slots of a foot block ("GFOOT"). A swing or stance enters SWING_* / STANCE_* / CLEAR_* when it ends, in the mode of the row that ends it,
 * and only when it also began inside the episode. */
enum {
  KBJ_GFOOT_TOUCHDOWNS   = 0,   /* rows on which the foot gains contact inside a running episode */
  KBJ_GFOOT_LIFTOFFS     = 1,   /* rows on which it loses contact */
  KBJ_GFOOT_SWING_N      = 2,   /* counted swings, */
  KBJ_GFOOT_SWING_SUM    = 3,   /* the sum of their durations, */
  KBJ_GFOOT_SWING_SUMSQ  = 4,   /* of the squares, */
  KBJ_GFOOT_SWING_MAX    = 5,   /* the longest */
  KBJ_GFOOT_STANCE_N     = 6,   /* the same of the counted stances */
  KBJ_GFOOT_STANCE_SUM   = 7,
  KBJ_GFOOT_STANCE_SUMSQ = 8,
  KBJ_GFOOT_STANCE_MAX   = 9,
  KBJ_GFOOT_CLEAR_SUM    = 10,  /* over the counted swings: sum of the clearance (m), */
  KBJ_GFOOT_CLEAR_SUMSQ  = 11,  /* of its square (taken in double), */
  KBJ_GFOOT_CLEAR_MAX    = 12,  /* the largest */
  KBJ_GFOOT_FORCE_SUM    = 13,  /* over the foot's contact rows: sum of the normal force (N), */
  KBJ_GFOOT_FORCE_MAX    = 14,  /* the largest */
  KBJ_GFOOT_CONTACT_ROWS = 15,  /* rows with the foot in contact */
  KBJ_GFOOT_SIZE         = 16
};
/* One env's totals of one call over all modes ("GENV" record, fp32): the seven row slots of a mode block, then per foot f eight slots at
 * KBJ_GENV_FOOT + KBJ_GENV_FOOT_STRIDE * f. */
enum {
  KBJ_GENV_FOOT        = 8,
  KBJ_GENV_TOUCHDOWNS  = 0,   /* foot slots: */
  KBJ_GENV_SWING_N     = 1,
  KBJ_GENV_SWING_SUM   = 2,
  KBJ_GENV_STANCE_N    = 3,
  KBJ_GENV_STANCE_SUM  = 4,
  KBJ_GENV_CLEAR_SUM   = 5,
  KBJ_GENV_CLEAR_MAX   = 6,
  KBJ_GENV_FORCE_MAX   = 7,
  KBJ_GENV_FOOT_STRIDE = 8,
  KBJ_GENV_SIZE        = 24
};

/* ---- actuator statistics (kbj_actuator_stats) ----
 * Per-env carry row ("AACC" record, fp32, owned by the caller on the device like the GACC rows; zeroed once). */
enum {
  KBJ_AACC_PREV    = 0,    /* [20] the action of the env's previous row */
  KBJ_AACC_RUNNING = 20,   /* 1 when a previous row exists and did not end its episode */
  KBJ_AACC_SIZE    = 24    /* 96-byte rows; the three spare floats at the end are left as they are */
};
/* One call's result ("ACT" record, doubles): KBJ_CMODE_COUNT mode blocks of KBJ_ACT_MODE_STRIDE slots (mode m's slot s at
 * m * KBJ_ACT_MODE_STRIDE + s): five head slots, then one block of KBJ_AJNT_SIZE joint slots per actuator u at KBJ_ACT_JOINT +
 * KBJ_AJNT_SIZE * u; then the episode counter. Every other slot is 0. */
enum {
  KBJ_ACT_ROWS          = 0,     /* rows of the mode */
  KBJ_ACT_PAIRS         = 1,     /* of them with a previous row in the same episode (the rows an action rate exists on) */
  KBJ_ACT_SPEED_SUM     = 2,     /* sum over the rows of the horizontal base speed (m/s, taken in double) */
  KBJ_ACT_ANY_TAU_ROWS  = 3,     /* rows with at least one actuator at its torque level */
  KBJ_ACT_ANY_STOP_ROWS = 4,     /* rows with at least one joint at a stop */
  KBJ_ACT_JOINT         = 8,     /* the first joint block */
  KBJ_ACT_MODE_STRIDE   = 256,
  KBJ_ACT_EPISODES      = 1536,  /* rows that start an episode (no previous row, or the previous row ended its episode) */
  KBJ_ACT_SIZE          = 1792
};
/* Slots of a joint block ("AJNT"). */
enum {
  KBJ_AJNT_TAU_SQ    = 0,    /* sum of tau^2 (N m)^2, taken in double */
  KBJ_AJNT_TAU_MAX   = 1,    /* largest |tau| */
  KBJ_AJNT_TAU_ROWS  = 2,    /* rows with |tau| >= tau_level[u] */
  KBJ_AJNT_VEL_SQ    = 3,    /* sum of omega^2 (rad/s)^2, taken in double */
  KBJ_AJNT_VEL_MAX   = 4,    /* largest |omega| */
  KBJ_AJNT_VEL_ROWS  = 5,    /* rows with |omega| >= vel_level[u] */
  KBJ_AJNT_POW_ABS   = 6,    /* sum of |P| (W), P = tau * omega in fp32 */
  KBJ_AJNT_POW_POS   = 7,    /* sum of max(P, 0): the work the motor puts in */
  KBJ_AJNT_POW_MAX   = 8,    /* largest |P| */
  KBJ_AJNT_STOP_ROWS = 9,    /* rows with q <= pos_lo[u] or q >= pos_hi[u] */
  KBJ_AJNT_DACT_SQ   = 10,   /* over the mode's PAIRS rows: sum of (a - a_prev)^2 (rad^2), taken in double */
  KBJ_AJNT_DACT_MAX  = 11,   /* largest |a - a_prev| */
  KBJ_AJNT_SIZE      = 12
};
/* One env's totals of one call over all modes ("AENV" record, fp32). */
enum {
  KBJ_AENV_ROWS          = 0,
  KBJ_AENV_PAIRS         = 1,
  KBJ_AENV_SPEED_SUM     = 2,
  KBJ_AENV_TAU_SQ        = 3,    /* the four sums below are over the env's rows and its 20 actuators */
  KBJ_AENV_POW_ABS       = 4,
  KBJ_AENV_POW_POS       = 5,
  KBJ_AENV_DACT_SQ       = 6,
  KBJ_AENV_ANY_TAU_ROWS  = 7,
  KBJ_AENV_ANY_STOP_ROWS = 8,
  KBJ_AENV_PEAK_FRAC     = 9,    /* largest |tau_u| / tau_level[u] over the env's rows and actuators */
  KBJ_AENV_PEAK_JOINT    = 10,   /* the u it was reached on (the lowest on a tie), -1 with no rows */
  KBJ_AENV_SIZE          = 12    /* one spare float, written as 0 */
};

/* ---- scripted pushes and push recovery (kbj_env_set_push, kbj_push_recovery) ----
 * The KBJ_ES_PUSH_NXT value that keeps the built-in ForcePushEvent from drawing: 2^24, an exactly countable fp32 (x - 1 is exact all the way
 * down), about 93 h of control steps at 50 Hz. */
#define KBJ_PUSH_NEVER 16777216.0f
/* Outcome of one env's scheduled push (kbj.h kbj_push_recovery). */
enum {
  KBJ_POUT_NONE        = 0,   /* no push scheduled (start row < 0) */
  KBJ_POUT_VOID        = 1,   /* the push says nothing: it starts outside the trajectory, or the env was not tracking / had just ended an episode before it */
  KBJ_POUT_FELL        = 2,   /* a failure (DONE < 0) inside the window */
  KBJ_POUT_RECOVERED   = 3,   /* hold_steps consecutive rows within the tolerances after the push ended */
  KBJ_POUT_UNRECOVERED = 4,   /* the whole window was seen, without a fall and without such a run */
  KBJ_POUT_CENSORED    = 5,   /* a time-out (DONE > 0) or the end of the trajectory cut the window before a decision */
  KBJ_POUT_COUNT       = 6
};
#define KBJ_NPEAK 4 /* peak errors kept per push: KBJ_TERR_LIN, _YAW, _TILT, _HEIGHT */
/* One env's result row ("PREC" record, fp32: whole numbers and maxima of fp32 inputs). A field that does not apply is -1. */
enum {
  KBJ_PREC_OUTCOME       = 0,   /* KBJ_POUT_* */
  KBJ_PREC_RECOVER_STEPS = 1,   /* RECOVERED: rows from the end of the push to the first row of the hold run */
  KBJ_PREC_FALL_STEPS    = 2,   /* FELL: rows from the start of the push to the failing row */
  KBJ_PREC_PEAK_LIN      = 3,   /* largest KBJ_TERR_LIN over the scanned rows (FELL, RECOVERED, UNRECOVERED, CENSORED), */
  KBJ_PREC_PEAK_YAW      = 4,   /* KBJ_TERR_YAW, */
  KBJ_PREC_PEAK_TILT     = 5,   /* KBJ_TERR_TILT, */
  KBJ_PREC_PEAK_HEIGHT   = 6,   /* KBJ_TERR_HEIGHT */
  KBJ_PREC_PEAK_ROW      = 7,   /* the first row at which PEAK_TILT is reached */
  KBJ_PREC_SIZE          = 8
};
/* One group's statistics ("PSTAT" record, doubles). A maximum over nothing is -1; spare slots are 0. */
enum {
  KBJ_PSTAT_COUNT      = 0,   /* [6] envs per outcome, KBJ_POUT_* order */
  KBJ_PSTAT_REC_SUM    = 6,   /* over the RECOVERED envs: sum of RECOVER_STEPS, */
  KBJ_PSTAT_REC_SUMSQ  = 7,   /* of its square, */
  KBJ_PSTAT_REC_MAX    = 8,   /* its maximum */
  KBJ_PSTAT_FALL_SUM   = 9,   /* over the FELL envs: sum of FALL_STEPS, */
  KBJ_PSTAT_FALL_SUMSQ = 10,  /* of its square, */
  KBJ_PSTAT_FALL_MAX   = 11,  /* its maximum */
  KBJ_PSTAT_PEAK_SUM   = 12,  /* [4] over the FELL, RECOVERED, UNRECOVERED and CENSORED envs: sum of each peak, KBJ_PREC_PEAK_LIN.. order, */
  KBJ_PSTAT_PEAK_MAX   = 16,  /* [4] its maximum */
  KBJ_PSTAT_SIZE       = 24
};

/* ---- command step response (kbj_step_response) ----
 * One row of the response signal ("SSIG" record, fp32): the base velocity in the robot's heading frame, the yaw rate, and the words of the
 * aux row the scan needs beside them. Channel k of a step (0 forward, 1 sideways, 2 yaw) is signal word k and command word k. */
enum {
  KBJ_SSIG_VX    = 0,   /* c qvel[0] + s qvel[1], (c, s) the trigonometry-free heading of the base quaternion, m/s */
  KBJ_SSIG_VY    = 1,   /* -s qvel[0] + c qvel[1], m/s */
  KBJ_SSIG_WZ    = 2,   /* qvel[5], rad/s (copied) */
  KBJ_SSIG_DONE  = 3,   /* KBJ_AUX_DONE of the row (copied) */
  KBJ_SSIG_CMD   = 4,   /* [3] KBJ_AUX_CMD + 0..2 of the row (copied) */
  KBJ_SSIG_SPARE = 7,   /* written 0 */
  KBJ_SSIG_SIZE  = 8
};
#define KBJ_NSCH 3 /* channels of a command step: forward, sideways, yaw */
/* Outcome of one env's scheduled command step (kbj.h kbj_step_response). Valid = KBJ_SOUT_FELL and above, as with KBJ_POUT_*. */
enum {
  KBJ_SOUT_NONE      = 0,   /* no step scheduled (row < 0) */
  KBJ_SOUT_VOID      = 1,   /* the step says nothing: outside the trajectory, no channel moved, or the env was not on its old command / had just ended an episode */
  KBJ_SOUT_FELL      = 2,   /* a failure (DONE < 0) inside the window */
  KBJ_SOUT_SETTLED   = 3,   /* hold_steps consecutive rows with every channel inside its band of the new command */
  KBJ_SOUT_UNSETTLED = 4,   /* the whole window was seen, without a fall and without such a run */
  KBJ_SOUT_CENSORED  = 5,   /* a time-out (DONE > 0), another command change, or the end of the trajectory cut the window before a decision */
  KBJ_SOUT_COUNT     = 6
};
/* One env's record ("SREC" record, fp32). A field that does not apply is -1; the spare words are 0. Times are in rows from the step row. */
enum {
  KBJ_SREC_OUTCOME      = 0,    /* KBJ_SOUT_* */
  KBJ_SREC_SETTLE_STEPS = 1,    /* SETTLED: rows from the step to the first row of the hold run */
  KBJ_SREC_FALL_STEPS   = 2,    /* FELL: rows from the step to the failing row */
  KBJ_SREC_ACTIVE       = 3,    /* valid outcomes: bit k set = channel k is active (its command moved by at least min_step[k]), held as a float */
  KBJ_SREC_TRAVEL_X     = 4,    /* valid outcomes: sum of the raw VX over the scanned rows, (m/s) x rows */
  KBJ_SREC_TRAVEL_Y     = 5,    /* of VY */
  KBJ_SREC_TRAVEL_YAW   = 6,    /* of WZ, (rad/s) x rows */
  KBJ_SREC_SPARE        = 7,    /* written 0 */
  KBJ_SREC_RISE         = 8,    /* [3] active channel: rows from the step to the first row at or beyond rise_level of the step, -1 if never */
  KBJ_SREC_OVER         = 11,   /* [3] active channel: largest excursion of the smoothed value beyond the new command, in the step's direction (>= 0) */
  KBJ_SREC_DEV          = 14,   /* [3] inactive channel: largest |smoothed value - command| (the cross-coupling) */
  KBJ_SREC_SPARE_TAIL   = 17,   /* [3] written 0 */
  KBJ_SREC_SIZE         = 20    /* 80-byte rows */
};
/* One group's statistics ("SSTAT" record, doubles). A maximum over nothing is -1; spare slots are 0. */
enum {
  KBJ_SSTAT_COUNT         = 0,    /* [6] envs per outcome, KBJ_SOUT_* order */
  KBJ_SSTAT_SETTLE_SUM    = 6,    /* over the SETTLED envs: sum of SETTLE_STEPS, */
  KBJ_SSTAT_SETTLE_SUMSQ  = 7,    /* of its square, */
  KBJ_SSTAT_SETTLE_MAX    = 8,    /* its maximum */
  KBJ_SSTAT_FALL_SUM      = 9,    /* over the FELL envs: sum of FALL_STEPS, */
  KBJ_SSTAT_FALL_SUMSQ    = 10,   /* of its square, */
  KBJ_SSTAT_FALL_MAX      = 11,   /* its maximum */
  KBJ_SSTAT_ACTIVE_N      = 12,   /* [3] per channel: valid envs with the channel active */
  KBJ_SSTAT_RISE_N        = 15,   /* [3] of them those with RISE >= 0, */
  KBJ_SSTAT_RISE_SUM      = 18,   /* [3] the sum of their RISE, */
  KBJ_SSTAT_RISE_MAX      = 21,   /* [3] its maximum */
  KBJ_SSTAT_OVER_SUM      = 24,   /* [3] over the valid envs with the channel active: sum of OVER, */
  KBJ_SSTAT_OVER_MAX      = 27,   /* [3] its maximum */
  KBJ_SSTAT_DEV_N         = 30,   /* [3] per channel: valid envs with the channel inactive, */
  KBJ_SSTAT_DEV_SUM       = 33,   /* [3] the sum of their DEV, */
  KBJ_SSTAT_DEV_MAX       = 36,   /* [3] its maximum */
  KBJ_SSTAT_TRAVEL_SUM    = 39,   /* [3] over the SETTLED envs: signed sum of TRAVEL_X, _Y, _YAW, */
  KBJ_SSTAT_TRAVEL_ABSMAX = 42,   /* [3] the largest magnitude */
  KBJ_SSTAT_SIZE          = 48    /* three spare slots, written 0 */
};

/* ---- command frequency response (kbj_frequency_response) ----
 * The signal is kbj_step_response's (KBJ_SSIG_*); channel k (0 forward, 1 sideways, 2 yaw) is signal word k and command word k.
 * Outcome of one env's scheduled lock-in window (kbj.h kbj_frequency_response). Valid = KBJ_FOUT_FELL and above, as with KBJ_SOUT_*. */
enum {
  KBJ_FOUT_NONE     = 0,   /* no window scheduled (row < 0) */
  KBJ_FOUT_VOID     = 1,   /* the schedule says nothing: a period that is no multiple of 4 in [4, 256], no such channel, no whole period, a window that
                              starts outside the trajectory or without its quarter period of lead rows, or an episode end in the lead rows */
  KBJ_FOUT_FELL     = 2,   /* a failure (DONE < 0) inside the window */
  KBJ_FOUT_MEASURED = 3,   /* the whole window was seen and the reference swung by at least min_amp */
  KBJ_FOUT_FLAT     = 4,   /* the whole window was seen, the reference did not swing: nobody moved the stick */
  KBJ_FOUT_CENSORED = 5,   /* a time-out (DONE > 0) or the end of the trajectory cut the window */
  KBJ_FOUT_COUNT    = 6
};
/* One env's record ("FREC" record, DOUBLES). Everything but OUTCOME is -1 for NONE and VOID; FALL_STEPS is -1 unless FELL. r = the driven
 * channel's command word of the row, d = the same word a quarter period earlier, y_k = VX, VY, WZ of the row. */
enum {
  KBJ_FREC_OUTCOME    = 0,    /* KBJ_FOUT_* */
  KBJ_FREC_ROWS       = 1,    /* rows accumulated: all sums below are over these */
  KBJ_FREC_FALL_STEPS = 2,    /* FELL: rows from the first measured row to the failing row */
  KBJ_FREC_CHANNEL    = 3,    /* the driven channel */
  KBJ_FREC_PERIOD     = 4,    /* the period in rows */
  KBJ_FREC_R_MIN      = 5,    /* smallest r (+inf over no comparable r), */
  KBJ_FREC_R_MAX      = 6,    /* greatest r (-inf over no comparable r) */
  KBJ_FREC_S_R        = 7,    /* sum r, */
  KBJ_FREC_S_D        = 8,    /* sum d, */
  KBJ_FREC_S_RR       = 9,    /* sum r r, */
  KBJ_FREC_S_DD       = 10,   /* sum d d, */
  KBJ_FREC_S_RD       = 11,   /* sum r d */
  KBJ_FREC_S_Y        = 12,   /* [3] sum y_k, */
  KBJ_FREC_S_YY       = 15,   /* [3] sum y_k y_k, */
  KBJ_FREC_S_YR       = 18,   /* [3] sum y_k r, */
  KBJ_FREC_S_YD       = 21,   /* [3] sum y_k d */
  KBJ_FREC_SIZE       = 24    /* 192-byte rows */
};
#define KBJ_FREC_NSUMS 17 /* the sums of a record: KBJ_FREC_S_R .. KBJ_FREC_SIZE - 1 */
/* One group's statistics ("FSTAT" record, doubles). A minimum or maximum over nothing is -1; spare slots are 0. */
enum {
  KBJ_FSTAT_COUNT    = 0,    /* [6] envs per outcome, KBJ_FOUT_* order */
  KBJ_FSTAT_FALL_SUM = 6,    /* over the FELL envs: sum of FALL_STEPS */
  KBJ_FSTAT_ROWS     = 7,    /* over the MEASURED envs: sum of ROWS, */
  KBJ_FSTAT_SUMS     = 8,    /* [17] of each sum, KBJ_FREC_S_R .. order, */
  KBJ_FSTAT_R_MIN    = 25,   /* the minimum of R_MIN, */
  KBJ_FSTAT_R_MAX    = 26,   /* the maximum of R_MAX */
  KBJ_FSTAT_SIZE     = 32    /* five spare slots, written 0 */
};

/* ---- scripted model perturbations and the robustness statistics (kbj_env_perturb, kbj_robustness) ----
 * One env's perturbation record ("PERT" record, fp32): how its model row (KBJ_EP_*) differs from the model blob's nominal values. Scales
 * multiply the model's word, additions are added to it; "valid" is what kbj_env_perturb accepts (every word read must be finite). */
enum {
  KBJ_PERT_MASS_SCALE     = 0,    /* every body's MASS and its three INERTIA words x s                                        (s > 0)  */
  KBJ_PERT_PAYLOAD        = 1,    /* kg added to the torso body's mass behind the scaling: a point mass at its COM            (>= 0)   */
  KBJ_PERT_MU_SCALE       = 2,    /* contact_mu x s                                                                           (s > 0)  */
  KBJ_PERT_ARMATURE_SCALE = 3,    /* every dof_armature x s                                                                   (s > 0)  */
  KBJ_PERT_FRICLOSS_SCALE = 4,    /* every dof_frictionloss x s                                                               (s >= 0) */
  KBJ_PERT_LATENCY        = 5,    /* action latency in substeps, a whole number; any negative value keeps KBJ_EP_LATENCY      (whole, or < 0) */
  KBJ_PERT_COM_SHIFT      = 6,    /* [3] metres added to the torso body's IPOS                                                (finite) */
  KBJ_PERT_SPARE          = 9,    /* [3] ignored, whatever they hold */
  KBJ_PERT_KP_SCALE       = 12,   /* [20] kp[u] x s                                                                           (s > 0)  */
  KBJ_PERT_KD_SCALE       = 32,   /* [20] kd[u] x s                                                                           (s >= 0) */
  KBJ_PERT_TAULIM_SCALE   = 52,   /* [20] tau_limit[u] x s                                                                    (s > 0)  */
  KBJ_PERT_ACTBIAS        = 72,   /* [20] copied into KBJ_EP_ACTBIAS, rad                                                     (finite) */
  KBJ_PERT_SIZE           = 92    /* 368-byte rows */
};
/* One env's record of kbj_robustness ("RREC" record, DOUBLES) over its rows t = 0 .. T-1. Spare words are 0. */
enum {
  KBJ_RREC_ROWS       = 0,    /* rows seen: T */
  KBJ_RREC_FALLS      = 1,    /* rows with DONE < 0 */
  KBJ_RREC_TIMEOUTS   = 2,    /* rows with DONE > 0 */
  KBJ_RREC_FIRST_FALL = 3,    /* the first row with DONE < 0, -1 without one */
  KBJ_RREC_SETTLED    = 4,    /* rows with KBJ_TERR_SETTLED != 0: the sums and maxima below are over these */
  KBJ_RREC_ERR_SUM    = 8,    /* [5] sum of the fp32 error taken into double, KBJ_TERR_* order (a NaN is taken as it is), */
  KBJ_RREC_ERR_SUMSQ  = 13,   /* [5] of its square, taken in double, */
  KBJ_RREC_ERR_MAX    = 18,   /* [5] its maximum: starts at -1, a NaN is never greater */
  KBJ_RREC_SIZE       = 24    /* 192-byte rows */
};
/* One group's statistics of kbj_robustness ("RSTAT" record, doubles). A minimum or maximum over nothing is -1; spare slots are 0. */
enum {
  KBJ_RSTAT_ENVS           = 0,    /* envs of the group */
  KBJ_RSTAT_FELL_ENVS      = 1,    /* of them those with FIRST_FALL >= 0 */
  KBJ_RSTAT_FALLS          = 2,    /* sum of FALLS, */
  KBJ_RSTAT_TIMEOUTS       = 3,    /* of TIMEOUTS, */
  KBJ_RSTAT_ROWS           = 4,    /* of ROWS */
  KBJ_RSTAT_FIRST_FALL_SUM = 5,    /* over the fell envs: sum of FIRST_FALL, */
  KBJ_RSTAT_FIRST_FALL_MIN = 6,    /* its minimum */
  KBJ_RSTAT_SETTLED        = 7,    /* sum of SETTLED */
  KBJ_RSTAT_ERR_SUM        = 8,    /* [5] sum of ERR_SUM, */
  KBJ_RSTAT_ERR_SUMSQ      = 13,   /* [5] of ERR_SUMSQ, */
  KBJ_RSTAT_ERR_MAX        = 18,   /* [5] the maximum of ERR_MAX */
  KBJ_RSTAT_SIZE           = 24
};

/* reward component order (train.py:1225-1256) */
enum {
  KBJ_REW_LINVEL = 0, KBJ_REW_ANGVEL, KBJ_REW_ROLL_PITCH, KBJ_REW_BASE_HEIGHT, KBJ_REW_ARM_POS,
  KBJ_REW_SINGLE_CONTACT, KBJ_REW_NO_CONTACT, KBJ_REW_FEET_AIRTIME, KBJ_REW_FEET_ORIENT,
  KBJ_REW_COM_DISTANCE, KBJ_REW_BASE_ACCEL, KBJ_REW_TORQUE
};

/* RNG stream ids (threefry2x32 key = (seed ^ stream * 0x9E3779B9, global env id)) */
enum {
  KBJ_RNG_RESET = 1, KBJ_RNG_RANDOMIZE = 2, KBJ_RNG_OBS_NOISE = 3, KBJ_RNG_COMMAND = 4,
  KBJ_RNG_ACTION = 5, KBJ_RNG_DROP = 6, KBJ_RNG_PUSH = 7, KBJ_RNG_INIT = 8, KBJ_RNG_SHUFFLE = 9
};

#ifdef __cplusplus
}
#endif
#endif /* KBJ_MODEL_H */
