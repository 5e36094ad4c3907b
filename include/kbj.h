/* kbj.h — C ABI of the MI355X-native K-Bot joystick hot path (rollout + PPO update).
 *
 * The reference has no FFI: its boundary is ksim's Python Task API (a `ksim.PPOTask` subclass,
 * train.py:1058) whose engine, rollout loop and PPO update run as jitted JAX programs. This
 * library is what a ksim-style host would bind instead of those programs; every entry point
 * cites the reference interface it replaces. The Python host layer
 * (kbot-joystick_amd/host) binds it with ctypes and re-exposes the Task API names.
 *
 * Conventions
 *  - All functions return 0 on success, <0 on error; kbj_last_error() gives the message.
 *    No exceptions cross the ABI, no torch types appear in signatures.
 *  - One kbj_ctx per (process, GPU). Not thread-safe; distinct contexts may be driven from
 *    distinct host threads. Work is enqueued on the hipStream_t given to kbj_create and is
 *    asynchronous unless stated otherwise.
 *  - Pointers named *_d are DEVICE pointers owned by the caller (e.g. torch tensor data_ptr());
 *    the library never frees caller memory. Pointers named *_h are host pointers.
 *  - Trajectory arrays are time-major, row-major: [T][N][dim] with dims/strides from kbj_model.h.
 *  - Multi-GPU: the library only produces/consumes flat fp32 buffers; the RCCL communicator is
 *    owned by the host (torch.distributed).
 */
#ifndef KBJ_H
#define KBJ_H

#include <stddef.h>
#include <stdint.h>
#include "kbj_model.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kbj_ctx kbj_ctx;

/* ---- lifetime ---------------------------------------------------------------------------- */
/* replaces: HumanoidWalkingTask.launch(config) set-up — get_mujoco_model / metadata / mjx.put_model
 * (train.py:1079-1089, 1760-1792). model_blob is a kbj_model produced by the spec compiler.
 * Model fields served (train.py:78-85): cfg->hidden_size in 1..512 (multiples of 64 run natively, above 256 on an untuned schedule; any other size runs zero padded to the
 * next one INSIDE the library - parameters, gradients, carries and trajectory start carries keep the caller's hidden_size layout and are
 * converted at every entry point, exact for this network), cfg->depth in 1..KBJ_MAX_DEPTH; anything else fails here. */
int kbj_create(kbj_ctx** out, const void* model_blob, size_t model_bytes, const kbj_config* cfg, int device, void* hip_stream);
int kbj_destroy(kbj_ctx* ctx);
const char* kbj_last_error(const kbj_ctx* ctx); /* ctx may be NULL: error of a failed kbj_create */
/* Host-only check of the sizes a configuration asks for (no device needed; kbj_create applies it first): 0 = served, -1 = refused with the
 * reason in `why`. Besides the range checks (hidden_size 1..512, depth 1..4, solver_newton 0 or 1: kbj_model.h) it refuses configurations whose largest
 * operand - the minibatch stash [rollout_len x batch_size][4 hidden_size | 476] or one control step's [num_envs][...] rows - reaches
 * 2 GiB: those arrays are fetched with 32-bit byte offsets. (The reference has no such limit: XLA addresses with 64 bits.) */
int kbj_check_config(const kbj_config* cfg, char* why, size_t why_bytes);
int kbj_sizeof_model(void);
int kbj_sizeof_config(void);
int kbj_sizeof_traj(void);    /* sizeof(kbj_traj), sizeof(kbj_carry): let a binding verify its struct mirrors */
int kbj_sizeof_carry(void);
int kbj_synchronize(kbj_ctx* ctx);

/* ---- environment (physics + task), SURVEY §8 rows a1-a3, a14-a22 -------------------------- */
/* replaces: ksim reset path — get_resets / get_physics_randomizers / initial commands and the first
 * get_observations call (train.py:1107-1132, 1146-1204, 724-766). Writes observation row 0. */
int kbj_env_reset_all(kbj_ctx* ctx, uint32_t seed, float* actor0_d, float* critic0_d, float* aux0_d);
/* replaces: one ksim engine control step = action latency/drop + ctrl_dt/dt x (PositionActuators.get_ctrl,
 * ForcePushEvent, mjx.step) + terminations + reset + command update + next observations
 * (train.py:1091-1105, 1134-1144, 1155-1222, 1258-1269, 1775-1781).
 * action_d [N][20]; aux_t_d [N][72] row of this step (completed); *_next_d rows of step t+1. */
int kbj_env_step(kbj_ctx* ctx, const float* action_d, float* aux_t_d, float* actor_next_d, float* critic_next_d, float* aux_next_d);
/* kbj_env_step plus the TERMINAL critic rows (kbj_config.gae_terminal_value; the reference's PPO stack bootstraps a time-out from the value of the
 * observation the episode ended in, which an env that resets in place never shows in row t+1): for every env whose episode ends in this step
 * (aux_t DONE != 0), row n of critic_term_d [N][ld_critic] receives the critic's observation of the state as it was BEFORE the reset - the
 * columns, expressions and derived data of a critic_next row (one device function writes both), the command of the ending episode, user and
 * pad columns zero. Rows of envs that go on are NOT written. Everything kbj_env_step writes is written bit for bit as kbj_env_step writes it;
 * the extra row draws no random number and moves no state. Its own kernels (env_step_term_kernel / env_step_term_cg_kernel): kbj_env_step's are
 * untouched. Not together with an armed kbj_env_record_state (refused; the record is disarmed). */
int kbj_env_step_terminal(kbj_ctx* ctx, const float* action_d, float* aux_t_d, float* actor_next_d, float* critic_next_d,
                          float* aux_next_d, float* critic_term_d /* [N][ld_critic] */);
/* One-shot: the NEXT kbj_env_step of this context also writes the step's state record (KBJ_QSTATE_*: qpos, qvel after the step and the
 * positions its last forward pass ran on) into qstate_t_d [N][KBJ_QSTATE_SIZE]. kbj_rollout does the same per step for kbj_traj.qstate_d;
 * this entry serves hosts that drive the steps themselves (user Termination / Observation / Command terms). NULL cancels. */
int kbj_env_record_state(kbj_ctx* ctx, float* qstate_t_d);
/* replaces: ksim's reset of the envs a Termination finished, for terminations decided OUTSIDE the step kernel - user-written terms in
 * the reference's protocol (`Termination.__call__(physics_data, curriculum_level) -> {-1, 0, 1}`, train.py:817) evaluated by the host on
 * the post-step record. mask_d [N] float: envs with a non-zero entry are re-initialised exactly as kbj_env_step re-initialises an env its
 * own terminations finish (same reset / randomiser / command streams, episode counter + 1) and their rows of the NEXT observation arrays
 * are rewritten; the others are untouched. The caller then writes the term's value into the step's KBJ_AUX_DONE column before
 * kbj_carry_reset / kbj_rewards / kbj_gae read it. */
int kbj_env_reset_where(kbj_ctx* ctx, const float* mask_d, float* actor_next_d, float* critic_next_d, float* aux_next_d);
/* replaces: the command update of a user-written Command term in the reference's protocol (`Command.initial_command(physics_data,
 * curriculum_level, rng)` / `Command.__call__(prev_command, physics_data, curriculum_level, rng)`, train.py:724, 768) evaluated by the host
 * between two control steps. cmd_d [N][16]; mask_d [N] float or NULL (= every env): the envs with a non-zero entry get cmd_d's row as
 * their joystick command - in the env state (the next kbj_env_step starts from it; run with command_mode = 1 so the kernel's own
 * switch draw does not replace it) and in the command columns + zero-command flag of the NEXT observation rows and aux record. */
int kbj_env_set_command(kbj_ctx* ctx, const float* mask_d, const float* cmd_d, float* actor_next_d, float* critic_next_d, float* aux_next_d);
/* replaces: a user-written Event term evaluated by the host between two control steps (the reference lists its events in get_events,
 * train.py:1134-1144; ksim's Event protocol itself is un-vendored, so the protocol of host/user_terms.py is this build's own). Writes the
 * event state the step kernel's ForcePushEvent reads at the start of every control step - nothing else: no observation, no aux row (a push
 * is in no observation). For every env whose mask_d [N] float entry is non-zero (NULL = every env):
 *   KBJ_ES_PUSH[0:6] = wrench_d's row [N][6]: force (N) then torque (N m), world frame, applied at the base body as the built-in event's;
 *   KBJ_ES_PUSH_REM  = steps_d[env];
 *   KBJ_ES_PUSH_NXT  = next_d[env] when next_d is given (NULL: untouched).
 * Both counters are floats holding whole numbers of CONTROL steps, as the kernel keeps them: steps = s pushes exactly the next s env
 * steps (the kernel counts REM down once per step while it is > 0 and applies the wrench on those steps); while REM > 0 it does not count
 * NXT down; when REM is 0 and NXT <= 0 the built-in event draws its own wrench, duration and interval. next = KBJ_PUSH_NEVER (kbj_model.h)
 * keeps the built-in event from drawing. An in-step reset (a termination inside kbj_env_step, kbj_env_reset_where) clears the wrench and REM
 * and re-arms the built-in schedule with a fresh NXT draw: a host that scripts pushes must write NXT again on the envs whose episode has
 * just started. Values are taken as they are; the host checks them (host/user_terms.py apply_events). Asynchronous on the context's stream;
 * other envs are untouched. A context with enable_pushes == 0 is refused with that reason: its step kernel ignores the event state. */
int kbj_env_set_push(kbj_ctx* ctx, const float* mask_d, const float* wrench_d /* [N][6] */, const float* steps_d /* [N] */, const float* next_d /* [N] or NULL */);
/* replaces: asking what a policy does on a robot that is NOT the model it trained on - the reference's physics randomisers
 * (get_physics_randomizers, train.py:1097-1132) draw such a robot at every reset, but nobody can hand them one: half the floor friction, a
 * payload on the torso, motors at 60 % torque, one weak leg. Writes a perturbed model row per env: for every env whose mask_d [N] float entry
 * is non-zero (NULL = every env) the physics and actuator columns of its KBJ_EP_* row are rewritten from the model blob's nominal values
 * and the env's record pert_d [N][KBJ_PERT_SIZE] (kbj_model.h KBJ_PERT_*), with m = the model, p = the record:
 *   MASS[b]       = m.body_mass[b] x p[MASS_SCALE]; for b = m.torso_body then + p[PAYLOAD]: fl(fl(mass x s) + payload), never fused;
 *   INERTIA[b][k] = m.body_inertia[b][k] x p[MASS_SCALE] (the payload is a point mass at the body's COM: no inertia of its own);
 *   IPOS[b][k]    = m.body_ipos[b][k] + (b = m.torso_body ? p[COM_SHIFT + k] : 0);
 *   ARMATURE[d]   = m.dof_armature[d] x p[ARMATURE_SCALE]; FRICLOSS[d] = m.dof_frictionloss[d] x p[FRICLOSS_SCALE];
 *   KP[u], KD[u], TAULIM[u] = m.kp[u] x p[KP_SCALE + u], m.kd[u] x p[KD_SCALE + u], m.tau_limit[u] x p[TAULIM_SCALE + u];
 *   ACTBIAS[u]    = p[ACTBIAS + u]; MU = m.contact_mu x p[MU_SCALE];
 *   CAP_POS = m.cap_pos + 0, CAP_HALF = m.cap_halflen, CAP_RAD = m.cap_radius: the model's capsules;
 *   LATENCY       = p[LATENCY] when that word is >= 0; a negative word keeps the row's own.
 * Every written word is ONE fp32 product or ONE fp32 sum rounded to nearest, never contracted: a float32 restatement on the host
 * reproduces every bit (tests/robustness_ref.py perturbed_row). Left exactly as they are: JPBIAS, PGBIAS, PGLAG (the per-episode sensor
 * draws), the zero tail behind MU, every other env, the env state (no KBJ_ES_* word) and every observation and aux row. The identity record
 * (scales 1, additions 0, LATENCY -1) gives the row the reset path writes with enable_randomizers = 0, latency and sensor draws kept.
 * No observation row needs rewriting: the actor's row (joint positions and speeds, projected gravity, gyroscope, command) depends on none of
 * the written columns. The critic's privileged columns that do (CINERT and its like, computed from MASS / INERTIA / IPOS) were written for
 * the next step by the last step or reset and stay as they are: they are one row stale, and right again from the next step's row on.
 * A record that breaks a "valid" condition of kbj_model.h, or holds a non-finite word among those read (the spare words are not), leaves
 * its env's row untouched. status_d: NULL, or [N] int32, overwritten for EVERY env: 0 = not masked, 1 = written, -1 = refused.
 * The step kernel reads the row afresh every control step (nothing derived from it is cached), so the new row acts from the next
 * kbj_env_step on. An in-step reset (a termination inside kbj_env_step, kbj_env_reset_where) redraws the whole row: a host that pins
 * parameters writes them again on the envs whose episode has just started, as kbj_env_set_push says of PUSH_NXT.
 * Asynchronous on the context's stream. Fails with a message, before anything is launched, on a NULL ctx or pert_d and on a pert_d that is
 * not 16-byte aligned. */
int kbj_env_perturb(kbj_ctx* ctx, const float* mask_d /* [N] or NULL = all */, const float* pert_d /* [N][KBJ_PERT_SIZE] */,
                    int32_t* status_d /* [N] or NULL */);
/* replaces: user-written Reset terms in the reference's protocol (`Reset.__call__(data, curriculum_level, rng) -> data`, train.py:833-844: the in-tree
 * PlaneXYPositionReset reads `data.qpos` and returns the data with a new one), evaluated by the host on the envs that have just been re-initialised
 * (by the step kernel's own terminations, kbj_env_reset_where or kbj_env_reset_all), AFTER the built-in resets of train.py:1146-1153 as in the
 * reference's list order. kbj_env_get_qstate copies every env's generalised positions / velocities into DEVICE arrays (qpos_d [N][27], qvel_d [N][26];
 * asynchronous, on the context's stream); kbj_env_set_qstate writes them back for the envs with a non-zero mask_d entry (NULL = all), clears their
 * solver warm start, re-runs the forward pass of the new state (kinematics, sensors, lagged projected gravity) and rewrites their NEXT observation
 * rows and aux record, exactly as the reset path does for the state it draws itself. Episode counter, randomised parameters and command are untouched. */
int kbj_env_get_qstate(kbj_ctx* ctx, float* qpos_d, float* qvel_d);
int kbj_env_set_qstate(kbj_ctx* ctx, const float* mask_d, const float* qpos_d, const float* qvel_d, float* actor_next_d, float* critic_next_d, float* aux_next_d);
/* state save/restore (checkpointing, tests): ep [N][KBJ_EP_SIZE], es [N][KBJ_ES_SIZE]; synchronous */
int kbj_env_get_state(kbj_ctx* ctx, float* ep_h, float* es_h);
int kbj_env_set_state(kbj_ctx* ctx, const float* ep_h, const float* es_h);
/* StatefulReward carries (train.py:135-136, 175-178: single-contact timer, feet airtime, previous contact flags) that kbj_rewards
 * keeps inside the context between rollouts: rc [N][KBJ_RC_SIZE]; synchronous. A resumed run needs them with ep/es. */
int kbj_env_get_reward_carry(kbj_ctx* ctx, float* rc_h);
int kbj_env_set_reward_carry(kbj_ctx* ctx, const float* rc_h);

/* ---- rewards, row a23 --------------------------------------------------------------------- */
/* replaces: get_rewards() stack evaluated over the trajectory (train.py:125-506, 1224-1256).
 * aux_d [T][N][72] -> reward_d [T][N] (sum of scale*term), comps_d [T][N][12] unscaled terms or NULL.
 * The StatefulReward carries persist inside the context across calls. */
int kbj_rewards(kbj_ctx* ctx, const float* aux_d, int T, float* reward_d, float* comps_d);

/* ---- actor-critic, rows a4-a11 ------------------------------------------------------------- */
/* Flat parameter vector layout (floats), equinox leaf order of Model(actor, critic)
 * (train.py:847-1046; convert.py:44-46):
 *   actor : input_proj.weight [H][65], input_proj.bias [H],
 *           rnns[l].weight_ih [4H][H], rnns[l].weight_hh [4H][H], rnns[l].bias [4H]   (l = 0..depth-1)
 *           output_proj.weight [40][H], output_proj.bias [40]
 *   critic: input_proj.weight [H][475], input_proj.bias [H], rnns[l]..., output_proj.weight [1][H], output_proj.bias [1]
 */
size_t kbj_param_count(const kbj_config* cfg);
size_t kbj_actor_param_count(const kbj_config* cfg);
/* replaces: get_model(InitParams(key)) (train.py:1278-1327): U(+-1/sqrt(fan_in)) init from a threefry stream */
int kbj_init_params(kbj_ctx* ctx, uint32_t seed, float* params_d);

/* The sagittal mirror of a PACKED observation row (mirror_obs / mirror_cmd / mirror_joints, train.py:1574-1756, applied to the rows
 * run_actor / run_critic pack, train.py:1351-1433) as the table the kernels use: out[k] = mul[k] * in[src[k]] + add[k] (the affine part
 * re-normalises joint positions whose source and destination joints have different biases / ranges). Host-only, needs no device:
 * fills KBJ_LD_ACTOR (critic = 0) or KBJ_LD_CRITIC (critic != 0) entries and returns that count (< 0 on error).
 * tests/test_ref_constants.py compares it with the table derived from the reference's source text. */
int kbj_mirror_table(const void* model_blob, size_t model_bytes, int critic, int32_t* src_h, float* mul_h, float* add_h);

/* Model carry (train.py:1049-1055, 1526-1543), device arrays owned by the caller:
 *   actor_hc_d / critic_hc_d [depth][2][N][H] (h then c per layer), lpf_d [N][20] */
typedef struct kbj_carry {
  float* actor_hc_d;
  float* critic_hc_d;
  float* lpf_d;
  /* mirror branches of the aux losses (train.py:1051-1055, 1463-1481); may be NULL when both mirror scales are 0 */
  float* actor_mirror_hc_d;
  float* critic_mirror_hc_d;
  float* lpf_mirror_d;
} kbj_carry;

/* replaces: sample_action() (train.py:1545-1572) for all envs at one control step, fused with what the
 * on-policy get_ppo_variables() pass would recompute for this step (log-prob, value; train.py:1435-1508):
 *   actor_obs_d [N][68], critic_obs_d [N][476] -> action_d [N][20], logp_d [N], value_d [N]; carry updated in place.
 * step_index seeds the Gaussian draw (RNG stream KBJ_RNG_ACTION); argmax!=0 returns the mode (train.py:1564). */
int kbj_policy_step(kbj_ctx* ctx, const float* params_d, const float* actor_obs_d, const float* critic_obs_d, kbj_carry* carry,
                    uint32_t seed, uint32_t step_index, int argmax, float* action_d, float* logp_d, float* value_d);
/* carry <- initial carry where done (train.py:1502-1506): done_d [N] float (aux KBJ_AUX_DONE column, stride in floats) */
int kbj_carry_reset(kbj_ctx* ctx, kbj_carry* carry, const float* done_d, int done_stride);
/* replaces: the bootstrap value every PPO stack takes at the end of a rollout - run_critic (train.py:1381-1433) on the observation that FOLLOWS the
 * last step (UPSTREAM MEMORY: ksim's GAE is un-vendored). The critic's value of ONE observation row critic_obs_d
 * [N][ld_critic] from the critic carries in `carry` (only carry->critic_hc_d is read): value_d [N]. Nothing the caller owns is written besides
 * value_d - the step runs on a copy of the carries inside the context, no net advances. The launches are those kbj_policy_step makes for
 * its critic, so value_d is bit-identical to what kbj_policy_step would write from the same carries and row. Needs a context created with
 * kbj_config.gae_tail_value = 1 (the carry copy is allocated then); call it where the carries are at rest: behind kbj_rollout, kbj_policy_step
 * or kbj_carry_reset. Hosts that drive the steps themselves call it behind their last kbj_carry_reset with observation row T and
 * kbj_traj.value_tail_d, BEFORE the update changes the parameters. */
int kbj_critic_value(kbj_ctx* ctx, const float* params_d, const float* critic_obs_d, const kbj_carry* carry, float* value_d);

/* The critic's value of the TERMINAL observations (kbj_config.gae_terminal_value), sparse: value_term_d[n] = 0.0f exactly where
 * done_d[n * done_stride] <= 0 (running, or failed: a failure bootstraps from nothing); where it is > 0 (time-out, or a user term's +1) the critic's
 * step - input projection of row n of critic_term_d [N][ld_critic], the LSTM layers from row n of carry->critic_hc_d, the value head - for that
 * one row, as matrix-vector products on the vector units, one workgroup per env (csrc/kbj_terminal_value.h). All N entries are written by every
 * call. Nothing else is written: carries and rows are read only. Call it between kbj_env_step_terminal of step t and kbj_carry_reset, when the
 * critic's carry is the one kbj_policy_step of step t left. Parameters and carries in the caller's layout at its own hidden_size (any size
 * kbj_create serves); works on every context, whatever its switches. Summation order differs from kbj_policy_step's matrix-core path: the same
 * value to fp32 rounding, not bit for bit. */
int kbj_critic_terminal_value(kbj_ctx* ctx, const float* params_d, const float* critic_term_d, const kbj_carry* carry,
                              const float* done_d, int done_stride, float* value_term_d /* [N] */);

/* ---- deployment, convert.py ------------------------------------------------------------------ */
/* replaces: the two functions convert.py exports for the robot (convert.py:74-119), served from the parameter vector itself. The deployed
 * function takes RAW sensor values and one FLAT carry per row, not the packed 68-float rows and plane carries of kbj_policy_step; it runs the
 * actor alone (no critic, no std head, no sampling: the action is dist.mode(), convert.py:119) as ONE launch, one workgroup per row
 * (csrc/kbj_deploy.h). N is the batch of THIS call, any positive number, independent of kbj_config.num_envs; the design range is N <= 64
 * (kbj_policy_step stays the throughput path). Flat carry of one row = ravel_pytree(Carry(actor_carry [depth][2][H], lpf_params))
 * (convert.py:46, 74-78): for each layer h [H] then c [H], then the 20 low-pass floats. */
typedef struct kbj_deploy_inputs {      /* convert.py:85-91, device arrays, N rows each */
  const float* joint_angles_d;          /* [N][20] rad, joint order of spec/constants.JOINT_NAMES */
  const float* joint_angular_velocities_d; /* [N][20] */
  const float* projected_gravity_d;     /* [N][3]  */
  const float* gyroscope_d;             /* [N][3]  */
  const float* command_d;               /* [N][16] order of COMMAND_NAMES */
} kbj_deploy_inputs;
/* replaces: metadata carry_size (convert.py:71): depth * 2 * hidden_size + 20 floats per row; host only, < 0 on a null argument */
int kbj_deploy_carry_size(const kbj_config* cfg);
/* replaces: init_fn (convert.py:74-82): the initial flat carry, zeros, carry_d [N][carry_size]; asynchronous on the context's stream */
int kbj_deploy_init(kbj_ctx* ctx, int N, float* carry_d);
/* replaces: step_fn (convert.py:84-119) for N rows: pack the 65-float observation from the raw inputs (convert.py:93-105; normalize_joint_pos /
 * normalize_joint_vel / encode_projected_gravity, train.py:1329-1349, with the arithmetic of the env kernel's observation rows), Actor.forward
 * (train.py:913-941) without the std head, action_d [N][20] = the low-pass filtered mean, carry_out_d = the new flat carry, whose last 20
 * floats are the action bit for bit. actor_params_d: the first kbj_actor_param_count(cfg) floats of a parameter vector in the layout above,
 * at the context's hidden_size (a full params_d is accepted; nothing is padded or copied). carry_out_d == carry_in_d is allowed (a workgroup
 * reads its whole row before it writes). A row's result is bitwise independent of N and of the row's position. Nothing is allocated per
 * call; asynchronous on the context's stream. A context with extra_obs_actor > 0 is refused: the contract has 65 inputs. */
int kbj_deploy_step(kbj_ctx* ctx, const float* actor_params_d, const kbj_deploy_inputs* in, int N,
                    const float* carry_in_d, float* carry_out_d, float* action_d /*[N][20]*/);

/* ---- rollout, §3.2 ------------------------------------------------------------------------- */
typedef struct kbj_traj {
  int32_t T, N;
  float* actor_obs_d;  /* [T+1][N][68]  row T = observation after the last step (row 0 of the next rollout) */
  float* critic_obs_d; /* [T+1][N][476] */
  float* aux_d;        /* [T+1][N][72]  */
  float* action_d;     /* [T][N][20] */
  float* logp_d;       /* [T][N] on-policy log-prob  */
  float* value_d;      /* [T][N] on-policy value     */
  float* reward_d;     /* [T][N] */
  float* carry0_actor_hc_d;  /* [depth][2][N][H] carry at the start of the trajectory (BPTT initial state) */
  float* carry0_critic_hc_d;
  float* carry0_lpf_d;       /* [N][20] */
  float* carry0_actor_mirror_hc_d;   /* mirror-branch carries at the start of the trajectory (NULL when the mirror losses are off) */
  float* carry0_critic_mirror_hc_d;
  float* carry0_lpf_mirror_d;
  float* reward_comps_d;     /* optional [T][N][12]: unscaled reward terms of the rollout (logging), or NULL */
  float* qstate_d;           /* optional [T][N][KBJ_QSTATE_SIZE]: qpos / qvel after every step + the positions its last forward pass ran on (the
                              * fields a ksim Trajectory carries for user reward terms: trajectory.qpos / .qvel / .xpos / .xquat, train.py:262-506), or NULL */
  float* value_tail_d;       /* optional [N]: the critic's value of observation row T from the carries after the last step (kbj_config.gae_tail_value:
                              * kbj_rollout writes it, kbj_gae bootstraps the last row from it), or NULL. Untouched while gae_tail_value is 0 */
} kbj_traj;
/* replaces: ksim's jitted rollout scan (vmap over envs, scan over T). Copies observation row T to row 0,
 * snapshots the carry, then T x (policy_step, env_step, carry_reset), then rewards. With kbj_config.gae_tail_value = 1 and a non-NULL
 * traj->value_tail_d it also runs the critic once more, on observation row T with a COPY of the carries the last carry reset left (the
 * caller's carries do not advance), with the rollout's parameters: exactly kbj_critic_value below. */
int kbj_rollout(kbj_ctx* ctx, const float* params_d, kbj_carry* carry, uint32_t seed, uint32_t first_step_index, kbj_traj* traj);
/* The buffer of terminal values, value_term_d [T][N] (kbj_config.gae_terminal_value; NULL unsets it): the following kbj_rollout calls of this
 * context write it, the following kbj_gae calls read it (hosts that drive the steps themselves fill row t with kbj_critic_terminal_value). A
 * context setting like kbj_set_advantage_sums, because kbj_traj cannot grow. With the switch on every step of kbj_rollout becomes (policy_step,
 * env_step_terminal, critic_terminal_value, carry_reset): the env phase runs its terminal form into a scratch of the context (allocated with
 * the switch on only), the sparse value kernel runs on the critic's lane in front of the critic's carry reset and writes row t. With the switch
 * on and no buffer set, kbj_rollout and kbj_gae fail before launching anything and the context stays usable; so does kbj_rollout with
 * traj->qstate_d (no env kernel writes both the state record and the terminal rows). Ignored with the switch off. */
int kbj_set_terminal_values(kbj_ctx* ctx, float* value_term_d);

/* replaces: `argmax=True` of sample_action during ksim's validation rollouts (train.py:1564, valid_every_n_steps train.py:1789): the following
 * kbj_rollout calls of this context act with the distribution's mode (the filtered mean) instead of a sample; the stored log-probs are those of the
 * mode. 0 restores sampling. (kbj_policy_step takes the flag per call.) */
int kbj_set_rollout_argmax(kbj_ctx* ctx, int argmax);

/* ---- episode metrics ------------------------------------------------------------------------ */
/* replaces: the episode metrics of the reference's logger (episodic return, episode length, which termination ended the episodes, the
 * per-episode sum of every reward term). That logger is ksim's, un-vendored: its metric list is UPSTREAM MEMORY, not a cited line.
 * An episode outlives a rollout (up to max_episode_steps = 600 control steps against 100), so the sums are carried per env ACROSS calls in
 * acc_d [N][KBJ_EACC_SIZE] fp32, device memory of the caller like kbj_carry (zero it once; save it with the env state), updated in place.
 * For every env n independently, for t = 0 .. T-1 in ascending order:
 *   acc[RETURN] += reward[t][n];  acc[LENGTH] += 1;  acc[TERM + k] += reward_comps[t][n][k] (skipped when traj->reward_comps_d is NULL);
 *   if aux[t][n][KBJ_AUX_DONE] != 0 the episode ends here: it enters the call's statistics with its cause (kbj_model.h KBJ_EPST_*: the
 *   sign of DONE, and for a failure the env kernel's own height test on the record's BASEZ / LFZ / RFZ) and the row's 14 sums return to 0.
 * The accumulations are plain fp32 adds in exactly this order (a float32 loop on the host reproduces acc_d bit for bit). stats_d
 * [KBJ_EPST_SIZE] doubles is OVERWRITTEN with the statistics of the episodes that finished inside this trajectory; the reduction over
 * the envs runs in double, in a fixed order, without atomics: the same inputs give bit-identical results on every call.
 * Reads traj->aux_d, traj->reward_d and, if present, traj->reward_comps_d (call it behind kbj_rollout / kbj_rewards and whatever the host
 * adds to the rewards); asynchronous on the context's stream. acc_d and reward_comps_d must be 16-byte aligned. */
int kbj_episode_stats(kbj_ctx* ctx, const kbj_traj* traj, float* acc_d, double* stats_d);

/* ---- command-tracking errors ----------------------------------------------------------------- */
/* replaces: watching the converted policy follow a joystick (the reference's README.md:48-52), as numbers. For every row (t, n) of
 * traj->aux_d, t = 0 .. T-1, the five tracking errors in fp32 and physical units (kbj_model.h KBJ_TERR_*): the error term of the
 * reference's reward class before its exp, in rewards_kernel's expressions (train.py:261-264, 274-290, 301-305, 316-330, 377-386), with
 * kbj_model.joint_bias and rew_standard_height / rew_foot_origin_height of the context's config.
 * Mode of a row (KBJ_CMODE_*), from its command alone with exact != 0.0f tests (-0.0 counts as zero): nz = which of cmd[0], cmd[1], cmd[2]
 * are non-zero, pose = any of cmd[3:16] non-zero. nz empty: STAND, or STAND_BEND with pose. nz non-empty with pose: OMNI. Exactly one of
 * nz without pose: FORWARD / SIDEWAYS / ROTATE. Otherwise OMNI.
 * Settled rows. acc_d [N][KBJ_TACC_SIZE] fp32 is device memory of the caller (zero it once; save it with the env state), updated in
 * place: the previous row's command, SINCE, RUNNING. For every env n independently, for t ascending:
 *   if RUNNING == 0, or cmd[k] != prev[k] for any k (float !=): since = 0 - the row starts an episode (RUNNING == 0: counted in
 *   KBJ_TRK_EPISODES) or changes the command inside one (counted in KBJ_TRK_CHANGES); otherwise since = min(SINCE + 1, 2^24).
 *   The row is settled when since >= settle_steps. Then prev = cmd, SINCE = since, RUNNING = (aux[t][n][KBJ_AUX_DONE] == 0).
 * The terminal row of an episode counts: aux[t] holds the state before the reset.
 * stats_d [KBJ_TRK_SIZE] doubles is OVERWRITTEN (kbj_model.h KBJ_TRK_*): per mode the rows, the settled rows and over the settled rows
 * the sum, the sum of squares (taken in double) and the fp32 maximum of each error; the reduction runs in double, in a fixed order,
 * without atomics: the same inputs give the same bytes on every call, with or without err_d.
 * err_d: NULL, or [T][N][KBJ_TERR_SIZE] fp32 that receives every row's errors, mode, settled flag and since.
 * Reads rows 0 .. T-1 of traj->aux_d only (neither rewards nor reward_comps_d); asynchronous on the context's stream. Fails with a message,
 * before anything is launched, on a NULL acc_d or stats_d, on an acc_d, err_d or traj->aux_d that is not 16-byte aligned, and on
 * settle_steps < 0. */
int kbj_tracking_stats(kbj_ctx* ctx, const kbj_traj* traj, int settle_steps, float* acc_d, double* stats_d, float* err_d);

/* ---- gait statistics --------------------------------------------------------------------------- */
/* replaces: watching HOW the converted policy walks (the viewer and a pair of eyes): swing and stance times, support shares, hops, foot
 * clearance, ground force and torque level, as numbers, split by the command mode of the row (KBJ_CMODE_*, the rule of kbj_tracking_stats).
 * The reference rewards this behaviour with single_contact, no_contact, feet_airtime and torque (train.py:138-213, 503-506); nobody reads
 * those in seconds, metres or newtons.
 * Row quantities. For row (t, n), a = aux[t][n], foot f = 0 left, 1 right:
 *   c[f] = a[KBJ_AUX_TOUCH + f] > 0.1f (rewards_kernel's own contact test; a NaN is no contact), F[f] = a[KBJ_AUX_TOUCH + f],
 *   z[0] = a[KBJ_AUX_LFZ], z[1] = a[KBJ_AUX_RFZ], mode = the row's KBJ_CMODE_*,
 *   q = sum over u = 0 .. 19, ascending, of (double)ctrl[u] * (double)ctrl[u], qmax = max over u of fabsf(ctrl[u]) (fmaxf, from 0).
 *   TOUCH is the observation BEFORE the step, the foot heights are those AFTER it: a one-row skew that is part of the definition.
 * Carry. acc_d [N][KBJ_GACC_SIZE] fp32 is device memory of the caller (zero it once; save it with the env state), updated in place: per
 * foot CON, RUN, VALID, ZST, PEAK, then RUNNING and LAST_TD (kbj_model.h KBJ_GACC_*); the spare floats are left as they are.
 * Scan. For every env n independently, for t ascending:
 *   1. ROWS[mode] += 1; DOUBLE, SINGLE or FLIGHT[mode] += 1 for c[0] + c[1] = 2, 1, 0; TORQUE_SQ[mode] += q; TORQUE_MAX[mode] = max(.., qmax).
 *   2. Per foot with c[f]: CONTACT_ROWS[mode][f] += 1; FORCE_SUM[mode][f] += (double)F[f]; FORCE_MAX[mode][f] = max(.., F[f]).
 *   3. If RUNNING == 0 the row starts an episode: EPISODES += 1; per foot CON = c[f], RUN = 1, VALID = 0, ZST = z[f], PEAK = 0;
 *      LAST_TD = -1. No events.
 *   4. Otherwise, per foot, left then right: if c[f] == CON, RUN = min(RUN + 1, 2^24). Otherwise a phase ends:
 *        touchdown (c[f]): TOUCHDOWNS[mode][f] += 1; if VALID: SWING_N += 1, SWING_SUM += RUN, SWING_SUMSQ += RUN^2, SWING_MAX = max(.., RUN),
 *          CLEAR_SUM += PEAK, CLEAR_SUMSQ += PEAK^2 (in double), CLEAR_MAX = max(.., PEAK); if LAST_TD == f: REPEATS[mode] += 1; LAST_TD = f.
 *        lift-off: LIFTOFFS[mode][f] += 1; if VALID: STANCE_N, STANCE_SUM, STANCE_SUMSQ, STANCE_MAX likewise from RUN.
 *        then CON = c[f], RUN = 1, VALID = 1, PEAK = 0.
 *   5. In either case, per foot: if c[f], ZST = z[f]; else PEAK = fmaxf(PEAK, z[f] - ZST).
 *   6. RUNNING = (a[KBJ_AUX_DONE] == 0).
 * So: a phase that began before the episode's first row has an unknown start - its end is counted as a touchdown or lift-off, its duration
 * and clearance are not; a phase the episode's end cuts is dropped; durations are in rows; clearance is the rise of the foot origin over its
 * height on the last contact row, which means the same on the terrain as on the plane. An event lands in the mode of the row that ends
 * the phase.
 * stats_d [KBJ_GAIT_SIZE] doubles is OVERWRITTEN (kbj_model.h KBJ_GAIT_*, KBJ_GFOOT_*): KBJ_CMODE_COUNT mode blocks, KBJ_GAIT_EPISODES, every
 * other slot 0. Every maximum is of a non-negative quantity: 0 over nothing. The reduction runs in double, in a fixed order (one env's rows
 * ascending, lanes in lane order, workgroups in block order), without atomics: the same inputs give the same bytes on every call, with or
 * without env_d.
 * env_d: NULL, or [N][KBJ_GENV_SIZE] fp32, overwritten: env n's totals of THIS call over all modes (kbj_model.h KBJ_GENV_*): ROWS, DOUBLE,
 * SINGLE, FLIGHT, REPEATS, TORQUE_SQ, TORQUE_MAX, 0, then per foot TOUCHDOWNS, SWING_N, SWING_SUM, STANCE_N, STANCE_SUM, CLEAR_SUM,
 * CLEAR_MAX, FORCE_MAX. Sums are accumulated in double in row order and rounded to fp32 once at the end: a float64 host loop in the same
 * order reproduces every word (tests/gait_ref.py).
 * Reads rows 0 .. T-1 of traj->aux_d only and writes no trajectory row; asynchronous on the context's stream. Fails with a message, before
 * anything is launched, on a NULL ctx, traj, acc_d or stats_d, on a trajectory without aux_d or positive T, N, and on an acc_d, env_d or
 * traj->aux_d that is not 16-byte aligned. */
int kbj_gait_stats(kbj_ctx* ctx, const kbj_traj* traj, float* acc_d, double* stats_d, float* env_d);

/* ---- actuator statistics ----------------------------------------------------------------------- */
/* replaces: asking what a policy demands of the motors before it goes onto the robot - torque against the limit, joint speed, mechanical
 * power, joint stops and the action rate - per actuator and split by the command mode of the row (KBJ_CMODE_*, the rule of
 * kbj_tracking_stats). The reference rewards this with its "sim2real" group, BaseAccelerationReward and TorqueReward (train.py:1253-1255),
 * and its metadata.json carries a soft_torque_limit per joint; nobody reads those per joint, in N m, rad/s or W.
 * Levels. kbj_actuator_levels holds the thresholds in physical units, per actuator in the order of spec/constants.JOINT_NAMES. They are
 * SETTINGS of the caller, not figures of the reference. tau_level and vel_level must be positive (vel_level may be +inf: it then counts
 * nothing), pos_lo <= pos_hi, nothing may be NaN.
 * Row quantities. For row (t, n) and actuator u = 0 .. 19, all in fp32 unless stated:
 *   tau   = aux[t][n][KBJ_AUX_CTRL + u]: the torque of the step's LAST substep, after the env's own clip at its (possibly randomised) limit,
 *   omega = qstate[t][n][KBJ_QSTATE_QVEL + 6 + u], q = qstate[t][n][KBJ_QSTATE_QPOS + 7 + u]: the joint AFTER the step; on a terminal row
 *           both hold the state before the reset,
 *   a     = action[t][n][u],
 *   P     = tau * omega, ONE fp32 product rounded to nearest. P is sampled at the control rate, from the last substep's torque and the
 *           end-of-step velocity: an ESTIMATE of the mechanical power, not an integral over the substeps,
 *   mode  = the row's KBJ_CMODE_* (from aux[t][n][KBJ_AUX_CMD ..]),
 *   speed = sqrt((double)vx * vx + (double)vy * vy) with vx, vy = aux[t][n][KBJ_AUX_QVEL + 0, 1], in double.
 *   at_tau[u] = fabsf(tau) >= tau_level[u]; over[u] = fabsf(omega) >= vel_level[u]; at_stop[u] = q <= pos_lo[u] || q >= pos_hi[u]
 *   (exact fp32 comparisons: a value ON the level counts, a NaN never does).
 * Carry. acc_d [N][KBJ_AACC_SIZE] fp32 is device memory of the caller (zero it once; save it with the env state), updated in place: PREV[u],
 * the previous row's action, and RUNNING; the three spare floats are left as they are.
 * Scan. For every env n independently, for t ascending, with m = mode:
 *   1. ROWS[m] += 1; SPEED_SUM[m] += speed; ANY_TAU_ROWS[m] += 1 if any at_tau[u]; ANY_STOP_ROWS[m] += 1 if any at_stop[u].
 *   2. Per actuator u: TAU_SQ[m][u] += (double)tau * (double)tau; TAU_MAX = fmaxf(.., fabsf(tau)); TAU_ROWS += at_tau[u];
 *      VEL_SQ += (double)omega * (double)omega; VEL_MAX = fmaxf(.., fabsf(omega)); VEL_ROWS += over[u];
 *      POW_ABS += (double)fabsf(P); POW_POS += (double)fmaxf(P, 0); POW_MAX = fmaxf(.., fabsf(P)); STOP_ROWS += at_stop[u].
 *   3. If RUNNING == 0 the row starts an episode: EPISODES += 1, and it has no action rate. Otherwise PAIRS[m] += 1 and per actuator
 *      d = a - PREV[u] (fp32): DACT_SQ[m][u] += (double)d * (double)d; DACT_MAX = fmaxf(.., fabsf(d)).
 *   4. PREV[u] = a; RUNNING = (aux[t][n][KBJ_AUX_DONE] == 0).
 * So the first row of an episode contributes no pair, within a call (DONE of the row before) and across calls (the carry's RUNNING).
 * stats_d [KBJ_ACT_SIZE] doubles is OVERWRITTEN (kbj_model.h KBJ_ACT_*, KBJ_AJNT_*): KBJ_CMODE_COUNT mode blocks of KBJ_ACT_MODE_STRIDE slots
 * (five head slots, then actuator u's KBJ_AJNT_SIZE slots at KBJ_ACT_JOINT + KBJ_AJNT_SIZE * u), then KBJ_ACT_EPISODES, every other slot 0.
 * Every maximum is of a non-negative quantity: 0 over nothing. The reduction runs in double, in a fixed order (one (env, actuator)'s rows
 * ascending - each run of consecutive rows that share a mode is summed by itself and the runs are added in row order -, envs in env order,
 * workgroups in block order), without atomics: the same inputs give the same bytes on every call, with or without env_d.
 * env_d: NULL, or [N][KBJ_AENV_SIZE] fp32, overwritten: env n's totals of THIS call over all modes (kbj_model.h KBJ_AENV_*). TAU_SQ,
 * POW_ABS, POW_POS and DACT_SQ are accumulated per actuator in double in row order, the 20 actuators are then added in ascending u from
 * 0.0, and the result is rounded to fp32 once; SPEED_SUM likewise over the rows. PEAK_FRAC = the largest fabsf(tau) / tau_level[u] (one fp32
 * division; fmaxf from 0) over rows and actuators, PEAK_JOINT the lowest u that reaches it (-1 with no rows); the spare float is 0. A
 * float64 host loop in the same order reproduces every word (tests/actuator_ref.py).
 * Reads rows 0 .. T-1 of traj->aux_d, traj->qstate_d (the state record: kbj_env_record_state, HumanoidWalkingTaskConfig.record_state) and
 * traj->action_d and writes no trajectory row; asynchronous on the context's stream; allocates nothing per call (the workgroup partials
 * live in the context, grown on first use). Fails with a message, before anything is launched or written, on a NULL ctx, traj, levels,
 * acc_d or stats_d ("null argument"), on a trajectory without aux_d, action_d or qstate_d (named as such, pointing to record_state) or
 * positive T, N, on an acc_d, env_d, aux_d, action_d or qstate_d that is not 16-byte aligned, on a level that is NaN or a tau_level /
 * vel_level that is not positive, and on pos_lo > pos_hi. levels is read before the call returns. */
typedef struct kbj_actuator_levels {   /* thresholds in physical units, per actuator, order of spec/constants.JOINT_NAMES */
  float tau_level[KBJ_NU];  /* N m:   a row counts as "at the torque level" where |tau_u| >= tau_level[u]  (> 0) */
  float vel_level[KBJ_NU];  /* rad/s: "over speed" where |omega_u| >= vel_level[u]                          (> 0, +inf allowed: counts nothing) */
  float pos_lo[KBJ_NU];     /* rad:   "at a joint stop" where q_u <= pos_lo[u] or q_u >= pos_hi[u]          (pos_lo <= pos_hi) */
  float pos_hi[KBJ_NU];
} kbj_actuator_levels;
int kbj_actuator_stats(kbj_ctx* ctx, const kbj_traj* traj, const kbj_actuator_levels* levels,
                       float* acc_d /* [N][KBJ_AACC_SIZE] */, double* stats_d /* [KBJ_ACT_SIZE] */, float* env_d /* [N][KBJ_AENV_SIZE] or NULL */);

/* ---- push recovery ---------------------------------------------------------------------------- */
/* replaces: shoving the robot and watching whether it stays up (what a locomotion policy is judged by before it goes on the robot), as
 * numbers: for one scheduled push per env, what became of it. Reads err_d [T][N][KBJ_TERR_SIZE], the per-row output of kbj_tracking_stats on
 * the same trajectory, the DONE column of rows 0 .. T-1 of traj->aux_d, and sched_d [N][2] int32 = (s, d): the push is applied during the d
 * rows s .. s + d - 1 (d < 0 counts as 0); s < 0 = no push for this env.
 * "Within" on row t: err[t][k] <= crit->tol[k] for every error k (KBJ_TERR_* order) whose tolerance is not +inf. A NaN error is not within;
 * a column whose tolerance is +inf is not looked at, whatever it holds (a NaN too). The tolerances are SETTINGS of the caller, not measured
 * thresholds.
 * Per env, with hold = crit->hold_steps >= 1 and window = crit->window_steps >= 0 (kbj_model.h KBJ_POUT_*, KBJ_PREC_*):
 *   s < 0: NONE.
 *   VOID: s >= T, or s < hold, or any of the rows [s - hold, s) is not within or has DONE != 0 (the env was not tracking its command, or
 *   had just ended an episode, when the push came: the push says nothing about recovery).
 *   Otherwise the rows t = s .. min(T, s + d + window) - 1 are scanned in order. On each row first the peaks: PEAK_LIN, PEAK_YAW, PEAK_TILT,
 *   PEAK_HEIGHT become the row's error where it is greater (they start at -1; a NaN is never greater), PEAK_ROW = t whenever PEAK_TILT
 *   rises. Then, in this order:
 *     1. DONE[t] < 0: FELL, FALL_STEPS = t - s. Stop.
 *     2. DONE[t] > 0: CENSORED. Stop.
 *     3. for t >= s + d the length of the run of consecutive within rows is kept (a row that is not within returns it to 0); when it reaches
 *        hold: RECOVERED, RECOVER_STEPS = (t - hold + 1) - (s + d), the rows from the end of the push to the first row of the run. Stop.
 *   Undecided at the end: CENSORED if s + d + window > T (the trajectory cut the window), else UNRECOVERED.
 * rec_d [N][KBJ_PREC_SIZE] fp32 is overwritten; fields that do not apply are -1 (all but the outcome for NONE and VOID). It holds whole
 * numbers and maxima of fp32 inputs: a host restatement reproduces it exactly (tests/push_ref.py).
 * stats_d: NULL, or [G][KBJ_PSTAT_SIZE] doubles, overwritten (spare slots 0): per group g the envs per outcome; over its RECOVERED envs the sum,
 * sum of squares and maximum of RECOVER_STEPS; over its FELL envs those of FALL_STEPS; over its FELL, RECOVERED, UNRECOVERED and CENSORED
 * envs the sum and maximum of each peak. A maximum over nothing is -1. group_d [N] int32 names every env's group (NULL: all in group 0; a
 * value outside [0, G) puts the env in no group), 1 <= G <= 256. A group's envs are combined in env order, in doubles, without atomics: a call
 * is bit-reproducible, with or without stats_d.
 * Asynchronous on the context's stream; crit is read before the call returns. Fails with a message, before anything is launched, on a NULL
 * traj, err_d, sched_d, crit or rec_d, on a trajectory without aux_d or positive T, N, on an err_d or rec_d that is not 16-byte aligned or a
 * sched_d that is not 8-byte aligned, on hold_steps < 1, window_steps < 0, a NaN tolerance, and with stats_d on G outside [1, 256]. */
typedef struct kbj_push_criteria {
  float tol[KBJ_NTERR];
  int32_t hold_steps, window_steps;
} kbj_push_criteria;
int kbj_push_recovery(kbj_ctx* ctx, const kbj_traj* traj, const float* err_d, const int32_t* sched_d, const kbj_push_criteria* crit,
                      float* rec_d, const int32_t* group_d, int G, double* stats_d);

/* ---- command step response -------------------------------------------------------------------- */
/* replaces: moving the stick and watching what the robot does (the first thing a joystick user feels), as numbers: for one scheduled
 * command change per env, how long the robot takes to reach the new command, how far it overshoots, when it settles, how far it travels
 * on the way, how much the channels that did not move are disturbed, and whether it falls. Channel k = 0 forward, 1 sideways, 2 yaw is
 * signal word k against command word k. The criteria are SETTINGS of the caller, not measured thresholds.
 * Stage 1, the signal. For every row (t, n), t = 0 .. T-1, with a = aux[t][n] and (w, x, y, z) = a[KBJ_AUX_BQUAT ..]:
 *   sn = 2 (w z + x y), cs = 1 - 2 (y^2 + z^2), h = sqrtf(sn^2 + cs^2); (c, s) = (cs / h, sn / h) if h > 0, else (1, 0)
 *   (the trigonometry-free heading of the env kernel's feet observation), and with (vx, vy) = a[KBJ_AUX_QVEL + 0 .. 1]:
 *   VX = c vx + s vy, VY = -s vx + c vy, WZ = a[KBJ_AUX_QVEL + 5], DONE = a[KBJ_AUX_DONE], CMD = a[KBJ_AUX_CMD + 0 .. 2] copied bit for
 *   bit, the spare word 0 (kbj_model.h KBJ_SSIG_*). Plain fp32: VX and VY agree with a double evaluation within rounding, not bit for bit.
 *   sig_d [T][N][KBJ_SSIG_SIZE] fp32 is OVERWRITTEN. Everything below is an exact function of sig_d.
 * Stage 2, per env n. s = sched_d[n] is the first row whose command is the new one; m = crit->smooth_steps, hold = crit->hold_steps,
 * window = crit->window_steps. All index arithmetic is in 64 bits: the schedule is the caller's.
 *   1. s < 0: NONE.
 *   2. c0 = CMD of row s - 1, c1 = CMD of row s, D_k = c1[k] - c0[k] in fp32, sg_k = +1 if D_k > 0, else -1.
 *      Channel k is active iff fabsf(D_k) >= min_step[k]. band_k = fmaxf(band_abs[k], band_frac * fabsf(D_k)),
 *      thr_k = rise_level * fabsf(D_k), each product rounded to fp32 once (round to nearest; no contraction).
 *      Every fmaxf here is taken as "replaced where the new value is greater": a NaN or a -0 never replaces the old value.
 *   3. The smoothed value S_k(t) = (float)((sum over u = max(s - hold, t - m + 1) .. t of (double)sig[u][n][k]) / (double)count): the sum
 *      ascends in u and is rounded once.
 *   4. VOID if any of: s >= T, or s < hold; a row in [s - hold, s) has DONE != 0; a row in [s - hold, s) has a CMD word that differs
 *      from c0 (float !=); no channel is active; |S_k(s - 1) - c0[k]| <= band_k is false for any of the three channels (the robot was
 *      not on its old command when the stick moved; a NaN is not within).
 *   5. Otherwise the rows t = s .. min(T, s + window) - 1 are scanned in order. On each row, in this order:
 *        1. DONE < 0: FELL, FALL_STEPS = t - s. Stop.
 *        2. DONE > 0: CENSORED. Stop.
 *        3. any CMD word != c1: CENSORED (the stick moved again). Stop.
 *        4. d_k = S_k(t) - c1[k] and p_k = sg_k (S_k(t) - c0[k]), each one fp32 subtraction, the sign applied by negation.
 *           Active channel: if RISE_k is still -1 and p_k >= thr_k, RISE_k = t - s; OVER_k = fmaxf(OVER_k, sg_k d_k), from 0.
 *           Inactive channel: DEV_k = fmaxf(DEV_k, fabsf(d_k)), from 0 (the cross-coupling).
 *        5. the travel sums, in double, add the RAW VX, VY, WZ of the row.
 *        6. within = fabsf(d_k) <= band_k for all three channels; run = within ? run + 1 : 0; when run reaches hold: SETTLED,
 *           SETTLE_STEPS = (t - hold + 1) - s. Stop.
 *   6. Undecided at the end: CENSORED if s + window > T (the trajectory cut the window), else UNSETTLED.
 *   7. rec_d [N][KBJ_SREC_SIZE] fp32 is OVERWRITTEN (kbj_model.h KBJ_SREC_*). TRAVEL_X, _Y, _YAW = the three double sums, each rounded
 *      to fp32 once, over the rows on which step 5.5 ran: up to and including the deciding row of a SETTLED env, up to the row in front
 *      of the one that stopped the scan in 5.1 - 5.3. Their unit is (m/s or rad/s) x rows: multiply by ctrl_dt. They are a path
 *      integral in the heading frame, and equal a displacement only while the heading barely turns. ACTIVE = sum of 2^k over the
 *      active channels. Fields that do not apply are -1: RISE / OVER of an inactive channel, DEV of an active one, and everything but
 *      OUTCOME for NONE and VOID. The spare words are 0.
 * stats_d: NULL, or [G][KBJ_SSTAT_SIZE] doubles, overwritten (spare slots 0; kbj_model.h KBJ_SSTAT_*): per group g the envs per outcome;
 * over its SETTLED envs the sum, sum of squares and maximum of SETTLE_STEPS; over its FELL envs those of FALL_STEPS; per channel over the
 * valid envs (FELL and above) with the channel active ACTIVE_N, the sum and maximum of OVER and, over those of them with RISE >= 0,
 * RISE_N and the sum and maximum of RISE; per channel over the valid envs with the channel inactive DEV_N and the sum and maximum of
 * DEV; over the SETTLED envs the signed sum and the largest magnitude of each TRAVEL word. A maximum over nothing is -1, and a NaN
 * never becomes one. group_d [N] int32 names every env's group (NULL: all in group 0; a value outside [0, G) puts the env in no group),
 * 1 <= G <= 256. A group's envs are combined in env order, in doubles, without atomics: the same inputs give the same bytes on every
 * call, with or without stats_d.
 * Reads rows 0 .. T-1 of traj->aux_d (40 bytes at the head of a row, three command words and DONE) and sched_d [N] int32; overwrites
 * sig_d, rec_d and stats_d. Asynchronous on the context's stream; crit is read before the call returns. Fails with a message, before
 * anything is launched, on a NULL ctx, traj, sched_d, crit, sig_d or rec_d, on a trajectory without aux_d or positive T, N, on a
 * traj->aux_d, sig_d or rec_d that is not 16-byte aligned, on smooth_steps outside [1, 32], hold_steps < 1, window_steps < 1,
 * rise_level outside (0, 1], a negative or NaN band_frac, band_abs or min_step, and with stats_d on G outside [1, 256]. The context
 * stays usable after such a failure. */
typedef struct kbj_step_criteria {
  float min_step[3];   /* a channel is active when |c1[k] - c0[k]| >= min_step[k] */
  float band_abs[3];   /* settle band floor per channel: m/s, m/s, rad/s */
  float band_frac;     /* settle band as a share of the step size */
  float rise_level;    /* in (0, 1] */
  int32_t smooth_steps, hold_steps, window_steps;   /* 1..32, >= 1, >= 1 */
} kbj_step_criteria;
int kbj_sizeof_step_criteria(void);   /* sizeof(kbj_step_criteria), for a binding's mirror */
int kbj_step_response(kbj_ctx* ctx, const kbj_traj* traj, const int32_t* sched_d /* [N] */, const kbj_step_criteria* crit,
                      float* sig_d /* [T][N][KBJ_SSIG_SIZE] */, float* rec_d /* [N][KBJ_SREC_SIZE] */,
                      const int32_t* group_d, int G, double* stats_d);

/* ---- command frequency response --------------------------------------------------------------- */
/* replaces: wiggling the stick at a steady rate and watching how far behind and how much smaller the robot's motion is (the gain and phase
 * lag a controls engineer asks of a velocity-tracking policy), as sums: for one scheduled window of whole periods per env, the lock-in
 * sums of the three response channels against the command the trajectory actually recorded and against the same command a quarter period
 * earlier. Gain, lag, delay, coherence and cross-coupling are formed from these sums on the host (host/frequency.py), none of it here.
 * Channel k = 0 forward, 1 sideways, 2 yaw is signal word k against command word k. min_amp is a SETTING of the caller, not a measured
 * threshold.
 * Stage 1, the signal: kbj_step_response's, bit for bit (the same kernel through the same launch). sig_d [T][N][KBJ_SSIG_SIZE] fp32 is
 *   OVERWRITTEN. Everything below is an exact function of sig_d.
 * Stage 2, per env n. sched_d[n] = {s, P, ch, K}: s the first measured row, P the period in rows, ch the driven channel, K the number of
 * whole periods measured; q = P / 4. All index arithmetic is in 64 bits, K * P in particular: the schedule is the caller's.
 * The reference r(t) = CMD[ch] of row t; its quadrature d(t) = r(t - q), the same word a quarter period earlier. No sine or cosine is
 * evaluated on the device: a host restatement reproduces every bit.
 *   1. s < 0: NONE.
 *   2. VOID if any of: P < 4, P > 256, P % 4 != 0, ch outside [0, 2], K < 1, s < q, s >= T, a lead row in [s - q, s) has DONE != 0.
 *   3. Otherwise the rows t = s .. min(T, s + K P) - 1 are scanned in order. On each row, in this order:
 *        1. DONE < 0: FELL, FALL_STEPS = t - s. Stop.
 *        2. DONE > 0: CENSORED. Stop.
 *        3. Accumulate, with y_0, y_1, y_2 = VX, VY, WZ of the row: R_MIN / R_MAX are replaced where r is smaller / greater (they start
 *           at +inf / -inf; a NaN never replaces them); ROWS += 1; the double sums S_R += r, S_D += d, S_RR += r r, S_DD += d d,
 *           S_RD += r d, and per channel k S_Y[k] += y_k, S_YY[k] += y_k y_k, S_YR[k] += y_k r, S_YD[k] += y_k d. Every operand is
 *           converted to double first (the product of two fp32 values is exact in double: fused or not gives the same sum); the adds
 *           ascend in t.
 *   4. At the end, for an env that has not stopped: s + K P > T: CENSORED (the trajectory cut the window). Else R_MAX - R_MIN >=
 *      min_amp[ch] (one fp32 subtraction; false for a NaN): MEASURED. Else FLAT: nobody moved the stick, a gain over nothing is noise.
 *   5. rec_d [N][KBJ_FREC_SIZE] DOUBLES is OVERWRITTEN (kbj_model.h KBJ_FREC_*): OUTCOME, ROWS, FALL_STEPS, CHANNEL, PERIOD, R_MIN, R_MAX,
 *      the 5 reference sums, the 12 response sums. The sums are kept as accumulated for FELL, CENSORED, FLAT and MEASURED alike: ROWS says
 *      over how many rows. Everything but OUTCOME is -1 for NONE and VOID; FALL_STEPS is -1 unless FELL.
 * stats_d: NULL, or [G][KBJ_FSTAT_SIZE] doubles, overwritten (spare slots 0; kbj_model.h KBJ_FSTAT_*): per group g the envs per outcome;
 * FALL_SUM over its FELL envs; over its MEASURED envs ONLY the sum of ROWS, of each of the 17 sums, the minimum of R_MIN and the maximum
 * of R_MAX. A minimum or maximum over nothing is -1. group_d [N] int32 names every env's group (NULL: all in group 0; a value outside
 * [0, G) puts the env in no group), 1 <= G <= 256. A group's envs are combined in env order, in doubles, without atomics: the same inputs
 * give the same bytes on every call, with or without stats_d. Pooling the raw sums is deliberate: where the envs of a group share s, P
 * and the command, the pooled sums are those of the concatenated windows.
 * Reads rows 0 .. T-1 of traj->aux_d (as kbj_step_response does) and sched_d [N][4] int32; overwrites sig_d, rec_d and stats_d.
 * Asynchronous on the context's stream; crit is read before the call returns. Fails with a message, before anything is launched, on a
 * NULL ctx, traj, sched_d, crit, sig_d or rec_d, on a trajectory without aux_d or positive T, N, on a traj->aux_d, sig_d or sched_d that
 * is not 16-byte aligned, on a rec_d or stats_d that is not 8-byte aligned, on a negative or NaN min_amp, and with stats_d on G outside
 * [1, 256]. The context stays usable after such a failure. */
typedef struct kbj_frequency_criteria {
  float min_amp[3];   /* the smallest swing R_MAX - R_MIN of the driven channel's command that counts as moved: m/s, m/s, rad/s */
} kbj_frequency_criteria;
int kbj_sizeof_frequency_criteria(void);   /* sizeof(kbj_frequency_criteria), for a binding's mirror */
int kbj_frequency_response(kbj_ctx* ctx, const kbj_traj* traj, const int32_t* sched_d /* [N][4] */, const kbj_frequency_criteria* crit,
                           float* sig_d /* [T][N][KBJ_SSIG_SIZE] */, double* rec_d /* [N][KBJ_FREC_SIZE] */,
                           const int32_t* group_d, int G, double* stats_d /* NULL or [G][KBJ_FSTAT_SIZE] */);

/* ---- robustness: survival and tracking per case ------------------------------------------------ */
/* replaces: running the policy on a robot that is not the model (kbj_env_perturb) and watching whether it stays up and still follows the
 * stick, as numbers: per env over the WHOLE trajectory how often it fell, when first, and how well the settled rows tracked; then the same
 * per group of envs (one group per case of a sweep). Reads err_d [T][N][KBJ_TERR_SIZE], the per-row output of kbj_tracking_stats on the same
 * trajectory (the five errors and the SETTLED flag), and the DONE column of rows 0 .. T-1 of traj->aux_d.
 * Per env n, for t = 0 .. T-1 in ascending order (kbj_model.h KBJ_RREC_*):
 *   ROWS += 1; DONE[t] < 0: FALLS += 1, and FIRST_FALL = t if it is still -1; DONE[t] > 0: TIMEOUTS += 1;
 *   if err[t][n][KBJ_TERR_SETTLED] != 0: SETTLED += 1 and per error k < KBJ_NTERR, with e = err[t][n][k]:
 *     ERR_SUM[k] += (double)e; ERR_SUMSQ[k] += (double)e * (double)e (exact in double: fused or not gives the same sum);
 *     ERR_MAX[k] = e where e is greater (it starts at -1; a NaN is never greater). A NaN error enters the sums as it is.
 * rec_d [N][KBJ_RREC_SIZE] DOUBLES is OVERWRITTEN; spare words are 0. A float64 host loop in the same order reproduces every word
 * (tests/robustness_ref.py).
 * stats_d: NULL, or [G][KBJ_RSTAT_SIZE] doubles, overwritten (spare slots 0; kbj_model.h KBJ_RSTAT_*): per group g its ENVS, those of them
 * that fell (FIRST_FALL >= 0), the sums of FALLS, TIMEOUTS, ROWS and SETTLED, over the fell envs the sum and the minimum of FIRST_FALL, the
 * sums of ERR_SUM and ERR_SUMSQ and the maximum of ERR_MAX. A minimum or maximum over nothing is -1. group_d [N] int32 names every env's
 * group (NULL: all in group 0; a value outside [0, G) puts the env in no group), 1 <= G <= 256. A group's envs are combined in env order, in
 * doubles, without atomics: the same inputs give the same bytes on every call, with or without stats_d.
 * Survival, falls per second and the mean errors are host arithmetic on these slots (host/robustness.py), none of it here.
 * Writes no trajectory row; asynchronous on the context's stream. Fails with a message, before anything is launched, on a NULL ctx, traj,
 * err_d or rec_d, on a trajectory without aux_d or positive T, N, on an err_d or rec_d that is not 16-byte aligned, and with stats_d on G
 * outside [1, 256]. The context stays usable after such a failure. */
int kbj_robustness(kbj_ctx* ctx, const kbj_traj* traj, const float* err_d /* [T][N][KBJ_TERR_SIZE] */, double* rec_d /* [N][KBJ_RREC_SIZE] */,
                   const int32_t* group_d, int G, double* stats_d /* NULL or [G][KBJ_RSTAT_SIZE] */);

/* ---- PPO update, rows a9, a12, a13 ---------------------------------------------------------- */
/* replaces: ksim GAE (gamma, lam: train.py:1769-1770). done from aux; adv_d/target_d [T][N].
 * Per env n, for t = T-1 .. 0, with d = aux[t][n][KBJ_AUX_DONE], v = value[t][n], r = reward[t][n] and A_T = 0:
 *   d < 0, or d > 0 with gae_bootstrap_truncation == 0:  delta = r - v                          A_t = delta   (terminal: the chain is cut)
 *   d > 0 with gae_bootstrap_truncation == 1:            delta = r + gamma v - v                A_t = delta   (truncation: cut, but bootstrapped)
 *   d > 0 with gae_terminal_value == 1:                  delta = r + gamma value_term[t][n] - v A_t = delta   (the same, from the terminal observation's value)
 *   d == 0, t < T-1:                                     delta = r + gamma value[t+1][n] - v    A_t = delta + gamma lam A_{t+1}
 *   d == 0, t == T-1:                                    delta = r + gamma vn - v               A_t = delta
 *                                                        vn = traj->value_tail_d[n] if gae_tail_value == 1, else v
 *   adv = A_t, target = A_t + v.
 * The switches are kbj_config fields, default 0 (this build's conventions: every non-zero DONE is terminal, V_T := V_{T-1}); with all at 0
 * the kernel of the earlier releases runs, bit for bit, and with gae_terminal_value at 0 the kernels of the two older switches do. At a
 * truncation v stands in for the value of the terminal observation, which observation row t+1 never shows (the env kernel resets in place:
 * that row already belongs to the next episode), unless gae_terminal_value = 1 (needs gae_bootstrap_truncation = 1): then value_term, the
 * [T][N] buffer of kbj_set_terminal_values, holds the critic's value of that observation (kbj_rollout / kbj_critic_terminal_value) and
 * stands there instead; without a buffer set the call fails like the NULL value_tail_d below. Either way a truncation in the LAST row
 * follows the truncation rule, not the tail rule (row T is a post-reset observation there). A user Termination term that writes +1 into the
 * DONE column gets the same treatment. gae_tail_value == 1 with traj->value_tail_d == NULL is an error: nothing is launched, the context
 * stays usable. tests/gae_ref.py restates this table in float64, tests/gae_terminal_ref.py its gae_terminal_value row. */
int kbj_gae(kbj_ctx* ctx, const kbj_traj* traj, float* adv_d, float* target_d);
/* replaces: the loss/grad of one minibatch: get_ppo_variables under grad (BPTT through T LSTM steps,
 * train.py:1435-1524) + ksim's clipped PPO loss. env_idx_d [B] int32 env indices of the minibatch.
 * When config.actor_mirror_loss_scale / critic_mirror_loss_scale are non-zero the mirror branches (train.py:1463-1481) run
 * under the gradient too and their aux losses are added; the carry / trajectory mirror arrays must then be non-NULL.
 * grad_d [P] flat gradient (overwritten), metrics_d [10]: loss, policy, value, entropy, clipfrac, kl, adv_mean, adv_std,
 * action_mirror_loss, value_mirror_loss */
int kbj_ppo_grad(kbj_ctx* ctx, const float* params_d, const kbj_traj* traj, const int32_t* env_idx_d, int B, const float* adv_d,
                 const float* target_d, float* grad_d, float* metrics_d);
/* replaces: get_ppo_variables(model, trajectory, model_carry, rng) (train.py:1510-1524) = the scan of _ppo_scan_fn (train.py:1435-1508)
 * WITHOUT taking gradients, for the B = config.batch_size envs env_idx_d names of ANY trajectory of the context's shape (one kbj_rollout
 * produced, or one reloaded into the same arrays): both nets run through the T steps from the trajectory's start carries with the carry
 * reset where `done` (train.py:1502-1506), and the per-step variables of PPOVariables come back as [T][B] arrays in env_idx order
 * (row t * B + b belongs to env env_idx_d[b]): log_probs of the stored actions (train.py:1452), values (:1455), entropy (:1486),
 * action_std [T][B][20] (:1487). entropy_d / action_std_d / action_mean_d may be NULL. The mirror aux losses are not evaluated here. */
typedef struct kbj_ppo_vars {
  float* logp_d;         /* [T][B] */
  float* value_d;        /* [T][B] */
  float* entropy_d;      /* [T][B] or NULL */
  float* action_std_d;   /* [T][B][20] or NULL */
  float* action_mean_d;  /* [T][B][20] or NULL: the filtered mean (the distribution's mode, train.py:936-939) */
} kbj_ppo_vars;
int kbj_ppo_forward(kbj_ctx* ctx, const float* params_d, const kbj_traj* traj, const int32_t* env_idx_d, int B, kbj_ppo_vars* out);
/* Next-minibatch hint (no reference counterpart: XLA schedules its whole update as one program): the NEXT kbj_ppo_grad / kbj_ppo_forward of
 * this context will be called with this trajectory and these indices (the same pointers). What that call gathers before its first
 * recurrence and that does not depend on the parameters - the actor's observation rows, the keep flags, the start carries - is queued now,
 * on a side lane behind everything enqueued on the context's stream so far, so it runs under the optimizer step between the two calls.
 * Purely a scheduling hint: results are identical with and without it; a call with other arguments simply ignores the prefetch. Call it
 * right after kbj_ppo_grad(k) with minibatch k + 1's indices. */
int kbj_ppo_prefetch(kbj_ctx* ctx, const kbj_traj* traj, const int32_t* env_idx_d);
/* Data-parallel overlap (no reference counterpart: the reference has no collective call site). After kbj_ppo_grad, work enqueued on
 * `hip_stream` behind this call starts once the ACTOR's slice of the gradient, grad_d[0, kbj_actor_param_count()), is final - about half
 * a millisecond before the call's own stream sees the whole gradient - so a host may all-reduce that slice on a second stream under the
 * critic's tail and the rest on the call's stream (host/task.py `overlap_allreduce`). */
int kbj_stream_wait_actor_grad(kbj_ctx* ctx, void* hip_stream);
/* Data-parallel variant of the advantage normalisation (ksim normalises the advantages of the batch it is given and
 * the reference has no multi-device call site to compare with): the following kbj_ppo_grad calls normalise with the statistics the caller
 * supplies - three doubles on the device, (sum adv, sum adv^2, sample count), e.g. the minibatch's sums all-reduced over the ranks so that
 * every rank normalises with the mean / variance of the GLOBAL minibatch - instead of their own minibatch's. NULL restores the default.
 * The pointer is read when kbj_ppo_grad runs (stream-ordered): fill it on the context's stream before the call. */
int kbj_set_advantage_sums(kbj_ctx* ctx, const double* sums_d);
/* Residency of the persistent recurrences (no reference counterpart: XLA has no persistent kernels). The T-step LSTM recurrences of
 * kbj_ppo_grad / kbj_ppo_forward are persistent launches whose workgroups hand tiles to each other, so a launch's whole grid must be resident:
 * *grid_wgs = workgroups of ONE recurrence launch at this configuration, *concurrent = launches this context keeps in flight at once (2: actor-
 * and critic-type net; 1 on the one-stream schedule), *slots = workgroups of the worst-fitting recurrence kernel the device holds (occupancy
 * query x CUs). kbj_create refuses a configuration with concurrent x grid > slots; a host that puts SEVERAL contexts (ranks) on one GPU must keep
 * the sum over them within slots (bench.py --share-gpu). A grid that cannot be placed fails within the wait bound (2 s, KBJ_SEQ_TIMEOUT_MS) and
 * every later launch of the call aborts at once: fail-stop in seconds, never a crawl. */
int kbj_recurrence_residency(kbj_ctx* ctx, int* grid_wgs, int* concurrent, int* slots);
/* replaces: optax.adamw + global-norm clip (train.py:1059-1077). step is 1-based. grad_scale multiplies the
 * gradient first (1/world_size after an all-reduce sum). */
int kbj_adamw_step(kbj_ctx* ctx, float* params_d, float* m_d, float* v_d, const float* grad_d, int64_t step, float grad_scale);
/* replaces: optax.cosine_decay_schedule feeding adamw (train.py:1067-1077): the host evaluates the schedule and sets the
 * learning rate used by the following kbj_adamw_step calls. Any finite value; a negative one moves the parameters ALONG the Adam direction,
 * which is what train.py:1074-1075 (scale_by_adam chained with scale_by_schedule, no sign flip) does as written. */
int kbj_set_learning_rate(kbj_ctx* ctx, float learning_rate);

/* per-launch timing of the dominant kernels, measured with HIP events on the context's stream (bench.py roofline) */
int kbj_profile_begin(kbj_ctx* ctx);
int kbj_profile_end(kbj_ctx* ctx, float* env_step_ms, int* env_step_launches, float* nn_ms, int* nn_launches);
/* per-kernel totals of the matrix-core kernels launched between kbj_profile_begin and kbj_profile_end: every launch is
 * bracketed by two HIP events on the stream it is launched on; flops = algorithmic 2*M*N*K of those launches */
typedef struct kbj_kernel_stat {
  char name[96];     /* kernel name as rocprofv3 prints it */
  int32_t launches;
  float total_ms;    /* sum of the launch durations */
  double flops;
} kbj_kernel_stat;
int kbj_profile_kernel_stats(kbj_ctx* ctx, kbj_kernel_stat* out, int capacity, int* count);

#ifdef __cplusplus
}
#endif
#endif /* KBJ_H */
