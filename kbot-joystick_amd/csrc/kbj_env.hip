// kbj_env.hip — HIP kernels + C-ABI entry points of the environment side of the hot path, everything that acts on env state:
// kbj_env_reset_all / kbj_env_step (one wavefront = one env, state in LDS; kbj_env_*.h), the masked resets, kbj_env_set_* / kbj_env_get_*,
// the reward carry's initialisation and its get / set. What reads a finished trajectory lives in kbj_traj_stats.hip.
#include <hip/hip_runtime.h>
#include "kbj_env_task.h"
#include "kbj_ctx.h"

using namespace kbj;

namespace {



// The constraint solver (kbj_config.solver_newton; kbj_env_phys.h phys_solve<CG>) is a compile-time parameter of every kernel that runs a
// forward pass, and each of them exists twice: the Newton ones keep their names and, instruction for instruction, the code they had before CG
// was served; the `_cg_` ones sit beside them. The host picks the symbol at launch from the context's config (KBJ_LAUNCH_SOLVER below);
// nothing branches on the solver inside a kernel. The three reset-type kernels are stamped out of a macro each rather than wrapped around
// an inlined body: the extra inlining level changes hipcc's register allocation and packing of the Newton form.
//
// grid = N workgroups of one wavefront; env state rows are read/written lane-contiguously (coalesced)
#define KBJ_ENV_RESET_KERNEL(NAME, CG) \
__global__ __launch_bounds__(64) void NAME(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed, \
                                                       float* __restrict__ ep, float* __restrict__ es, float* actor0, float* critic0, float* aux0) { \
  __shared__ KbjShared S; \
  const int env = blockIdx.x; \
  PFOR(k, (int)(sizeof(KbjModelLds) / sizeof(float))) reinterpret_cast<float*>(&S.mc)[k] = mc[k]; \
  PFOR(k, (int)(sizeof(PhysConst) / sizeof(float))) reinterpret_cast<float*>(&S.pc)[k] = reinterpret_cast<const float*>(pcp)[k]; \
  PFOR(k, KBJ_ES_SIZE) S.es[k] = 0; \
  PFOR(k, 12) S.zrow[k] = 0; \
  KBJ_SYNC(); \
  Rng rng{seed, (uint32_t)(c->env_id_offset + env)}; \
  const PhysConst& pc = S.pc; \
  task_reset<CG>(S, *m, *c, pc, rng); \
  task_write_obs(S, *m, *c, rng, actor0 + (size_t)env * KBJ_LD_OF(KBJ_NOBS_ACTOR + c->extra_obs_actor), critic0 + (size_t)env * KBJ_LD_OF(KBJ_NOBS_CRITIC + c->extra_obs_critic), aux0 + (size_t)env * KBJ_AUX_SIZE); \
  PFOR(k, KBJ_EP_SIZE) ep[(size_t)env * KBJ_EP_SIZE + k] = S.ep[k]; \
  PFOR(k, KBJ_ES_SIZE) es[(size_t)env * KBJ_ES_SIZE + k] = S.es[k]; \
}
KBJ_ENV_RESET_KERNEL(env_reset_kernel, false)
KBJ_ENV_RESET_KERNEL(env_reset_cg_kernel, true)

// re-initialise the envs whose mask entry is non-zero, exactly as env_step_kernel does for an env its own terminations finish (same
// task_reset / task_write_obs on the env's state row: the episode counter advances, the randomisers, reset distributions and the first
// command are drawn from the env's streams) and rewrite their next observation rows; other envs are untouched. For terminations decided
// OUTSIDE the kernel (user-written Termination terms on the host, train.py:817 protocol).
#define KBJ_ENV_RESET_WHERE_KERNEL(NAME, CG) \
__global__ __launch_bounds__(64) void NAME(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed, \
                                                             float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ mask, float* actor_next, \
                                                             float* critic_next, float* aux_next) { \
  __shared__ KbjShared S; \
  const int env = blockIdx.x; \
  if (mask[env] == 0.0f) return;     /* uniform over the workgroup */ \
  PFOR(k, (int)(sizeof(KbjModelLds) / sizeof(float))) reinterpret_cast<float*>(&S.mc)[k] = mc[k]; \
  PFOR(k, (int)(sizeof(PhysConst) / sizeof(float))) reinterpret_cast<float*>(&S.pc)[k] = reinterpret_cast<const float*>(pcp)[k]; \
  PFOR(k, KBJ_EP_SIZE) S.ep[k] = ep[(size_t)env * KBJ_EP_SIZE + k]; \
  PFOR(k, KBJ_ES_SIZE) S.es[k] = es[(size_t)env * KBJ_ES_SIZE + k]; \
  PFOR(k, 12) S.zrow[k] = 0; \
  KBJ_SYNC(); \
  Rng rng{seed, (uint32_t)(c->env_id_offset + env)}; \
  const PhysConst& pc = S.pc; \
  task_reset<CG>(S, *m, *c, pc, rng); \
  task_write_obs(S, *m, *c, rng, actor_next + (size_t)env * KBJ_LD_OF(KBJ_NOBS_ACTOR + c->extra_obs_actor), critic_next + (size_t)env * KBJ_LD_OF(KBJ_NOBS_CRITIC + c->extra_obs_critic), aux_next + (size_t)env * KBJ_AUX_SIZE); \
  PFOR(k, KBJ_EP_SIZE) ep[(size_t)env * KBJ_EP_SIZE + k] = S.ep[k]; \
  PFOR(k, KBJ_ES_SIZE) es[(size_t)env * KBJ_ES_SIZE + k] = S.es[k]; \
}
KBJ_ENV_RESET_WHERE_KERNEL(env_reset_where_kernel, false)
KBJ_ENV_RESET_WHERE_KERNEL(env_reset_where_cg_kernel, true)

// user-written Reset terms (train.py:833-844 protocol): the generalised state of every env as device arrays ...
__global__ __launch_bounds__(256) void env_get_qstate_kernel(int N, const float* __restrict__ es, float* __restrict__ qpos, float* __restrict__ qvel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, env = i / 64, k = i % 64;
  if (env >= N) return;
  if (k < KBJ_NQ) qpos[(size_t)env * KBJ_NQ + k] = es[(size_t)env * KBJ_ES_SIZE + KBJ_ES_QPOS + k];
  if (k < KBJ_NV) qvel[(size_t)env * KBJ_NV + k] = es[(size_t)env * KBJ_ES_SIZE + KBJ_ES_QVEL + k];
}
// ... and back for the masked envs: new positions / velocities, cleared warm start, then what task_reset does behind the state it draws itself -
// one forward pass (PD on the held action, kinematics, sensors), the lagged projected gravity re-seeded, the next observation rows rewritten
#define KBJ_ENV_SET_QSTATE_KERNEL(NAME, CG) \
__global__ __launch_bounds__(64) void NAME(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed, \
                                                            float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ mask, const float* __restrict__ qpos, \
                                                            const float* __restrict__ qvel, float* actor_next, float* critic_next, float* aux_next) { \
  __shared__ KbjShared S; \
  const int env = blockIdx.x; \
  if (mask && mask[env] == 0.0f) return;     /* uniform over the workgroup */ \
  PFOR(k, (int)(sizeof(KbjModelLds) / sizeof(float))) reinterpret_cast<float*>(&S.mc)[k] = mc[k]; \
  PFOR(k, (int)(sizeof(PhysConst) / sizeof(float))) reinterpret_cast<float*>(&S.pc)[k] = reinterpret_cast<const float*>(pcp)[k]; \
  PFOR(k, KBJ_EP_SIZE) S.ep[k] = ep[(size_t)env * KBJ_EP_SIZE + k]; \
  PFOR(k, KBJ_ES_SIZE) S.es[k] = es[(size_t)env * KBJ_ES_SIZE + k]; \
  PFOR(k, 12) S.zrow[k] = 0; \
  KBJ_SYNC(); \
  PFOR(k, KBJ_NQ) S.es[KBJ_ES_QPOS + k] = qpos[(size_t)env * KBJ_NQ + k]; \
  PFOR(k, KBJ_NV) { S.es[KBJ_ES_QVEL + k] = qvel[(size_t)env * KBJ_NV + k]; S.es[KBJ_ES_WARM + k] = 0; } \
  KBJ_SYNC(); \
  PFOR(w, 1) {   /* a unit base quaternion whatever the term returned */ \
    float* q = S.es + KBJ_ES_QPOS + 3; \
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); \
    if (!(n > 0)) { q[0] = 1; q[1] = q[2] = q[3] = 0; } \
    else if (fabsf(n - 1.0f) > 1e-6f) { q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n; }     /* (a term that leaves the state alone leaves its bits alone) */ \
    S.pushing = 0; \
  } \
  KBJ_SYNC(); \
  Rng rng{seed, (uint32_t)(c->env_id_offset + env)}; \
  const PhysConst& pc = S.pc; \
  task_pd(S, S.es + KBJ_ES_ACT_PREV); \
  phys_forward<CG>(S, S.mc, pc); \
  PFOR(k, 3) S.es[KBJ_ES_PGLAG + k] = S.pg[k]; \
  KBJ_SYNC(); \
  task_write_obs(S, *m, *c, rng, actor_next + (size_t)env * KBJ_LD_OF(KBJ_NOBS_ACTOR + c->extra_obs_actor), critic_next + (size_t)env * KBJ_LD_OF(KBJ_NOBS_CRITIC + c->extra_obs_critic), aux_next + (size_t)env * KBJ_AUX_SIZE); \
  PFOR(k, KBJ_ES_SIZE) es[(size_t)env * KBJ_ES_SIZE + k] = S.es[k]; \
}
KBJ_ENV_SET_QSTATE_KERNEL(env_set_qstate_kernel, false)
KBJ_ENV_SET_QSTATE_KERNEL(env_set_qstate_cg_kernel, true)

// overwrite the joystick command of the envs whose mask entry is non-zero (mask == nullptr: all envs): the env's state row (the next step's
// rewards and its command-switch draw start from it) and the command columns of the NEXT observation rows + aux record, zero-command flag
// included — what task_write_obs wrote there from the kernel's own command. One thread per (env, command slot).
__global__ __launch_bounds__(256) void env_set_command_kernel(int N, int lda, int ldc, float* __restrict__ es, const float* __restrict__ mask, const float* __restrict__ cmd, float* actor_next,
                                                              float* critic_next, float* aux_next) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, env = i / KBJ_NCMD, k = i % KBJ_NCMD;
  if (env >= N || (mask && mask[env] == 0.0f)) return;
  const float* c = cmd + (size_t)env * KBJ_NCMD;
  const float v = c[k];
  es[(size_t)env * KBJ_ES_SIZE + KBJ_ES_CMD + k] = v;
  actor_next[(size_t)env * lda + KBJ_OBS_CMD + k] = v;
  critic_next[(size_t)env * ldc + KBJ_OBS_CMD + k] = v;
  aux_next[(size_t)env * KBJ_AUX_SIZE + KBJ_AUX_CMD + k] = v;
  if (k == 0) {
    const float zc = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) < 1e-3f ? 1.0f : 0.0f;
    actor_next[(size_t)env * lda + KBJ_OBS_ZEROCMD] = zc;
    critic_next[(size_t)env * ldc + KBJ_OBS_ZEROCMD] = zc;
  }
}

// overwrite the push-event state of the envs whose mask entry is non-zero (mask == nullptr: all envs): the wrench, the control steps it is
// still applied for and, when `next` is given, the control steps until the built-in event draws again - the words task_step's ForcePushEvent
// reads at the start of the next control step. No observation row holds any of it. One thread per (env, slot): slots 0-5 the wrench, 6 REM, 7 NXT.
__global__ __launch_bounds__(256) void env_set_push_kernel(int N, float* __restrict__ es, const float* __restrict__ mask, const float* __restrict__ wrench, const float* __restrict__ steps,
                                                           const float* __restrict__ next) {
  static_assert(KBJ_ES_PUSH_REM == KBJ_ES_PUSH + 6 && KBJ_ES_PUSH_NXT == KBJ_ES_PUSH + 7, "the push block of the env state row");
  const int i = blockIdx.x * blockDim.x + threadIdx.x, env = i / 8, k = i % 8;
  if (env >= N || (mask && mask[env] == 0.0f)) return;
  if (k == 7 && !next) return;
  es[(size_t)env * KBJ_ES_SIZE + KBJ_ES_PUSH + k] = k < 6 ? wrench[(size_t)env * 6 + k] : k == 6 ? steps[env] : next[env];
}

// one word of a perturbation record against the "valid" column of kbj_model.h KBJ_PERT_*: the spare words are not read; every other word is
// finite; scales are positive (KD and FRICLOSS: not negative), the payload is not negative, the latency is negative or a whole number
__device__ inline bool pert_word_valid(int i, float v) {
  if (i >= KBJ_PERT_SPARE && i < KBJ_PERT_KP_SCALE) return true;
  if (!(fabsf(v) < INFINITY)) return false;                    // a NaN or an infinity
  if (i == KBJ_PERT_MASS_SCALE || i == KBJ_PERT_MU_SCALE || i == KBJ_PERT_ARMATURE_SCALE || (i >= KBJ_PERT_KP_SCALE && i < KBJ_PERT_KD_SCALE) ||
      (i >= KBJ_PERT_TAULIM_SCALE && i < KBJ_PERT_ACTBIAS))
    return v > 0.0f;
  if (i == KBJ_PERT_PAYLOAD || i == KBJ_PERT_FRICLOSS_SCALE || (i >= KBJ_PERT_KD_SCALE && i < KBJ_PERT_TAULIM_SCALE)) return v >= 0.0f;
  if (i == KBJ_PERT_LATENCY) return v < 0.0f || v == floorf(v);
  return true;                                                 // COM_SHIFT, ACTBIAS: finite
}

// One fp32 product / one fp32 sum, rounded to nearest, that no pass fuses with its neighbour. __fmul_rn / __fadd_rn are plain * and + to
// this compiler and carry their header's contraction licence into the caller: the torso's scaled mass plus the payload became one fused
// multiply-add and missed the two-rounding value by an ulp on one env in ten. Here the licence is withdrawn where the operation is written.
__device__ inline float pert_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ inline float pert_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// rewrite the physics and actuator columns of the KBJ_EP row of the envs whose mask entry is non-zero (mask == nullptr: all envs) from the
// model's nominal values and the env's perturbation record (kbj.h kbj_env_perturb, word for word): every written word is one pert_mul or one
// pert_add, so nothing is contracted and a float32 restatement reproduces every bit. JPBIAS, PGBIAS, PGLAG and the tail behind MU are not
// touched, LATENCY only for a record word >= 0. An invalid record leaves the row alone. One wavefront per env: lanes 0 .. 22 fetch the
// record as 16-byte pieces into LDS and judge their own words, one vote decides, then the lanes share the row's 346 words.
__global__ __launch_bounds__(64) void env_perturb_kernel(int N, const kbj_model* __restrict__ m, float* __restrict__ ep, const float* __restrict__ mask, const float* __restrict__ pert,
                                                         int32_t* __restrict__ status) {
  static_assert(KBJ_PERT_SIZE % 4 == 0 && KBJ_PERT_SIZE / 4 <= 64, "a record is fetched as 16-byte pieces, one per lane");
  static_assert(KBJ_EP_IPOS == 0 && KBJ_EP_MASS == 3 * KBJ_NBODY && KBJ_EP_INERTIA == KBJ_EP_MASS + KBJ_NBODY && KBJ_EP_ARMATURE == KBJ_EP_INERTIA + 3 * KBJ_NBODY &&
                KBJ_EP_FRICLOSS == KBJ_EP_ARMATURE + KBJ_NV && KBJ_EP_CAP_POS == KBJ_EP_FRICLOSS + KBJ_NV && KBJ_EP_CAP_HALF == KBJ_EP_CAP_POS + 3 * KBJ_NCAP &&
                KBJ_EP_CAP_RAD == KBJ_EP_CAP_HALF + KBJ_NCAP && KBJ_EP_KP == KBJ_EP_CAP_RAD + KBJ_NCAP && KBJ_EP_KD == KBJ_EP_KP + KBJ_NU && KBJ_EP_TAULIM == KBJ_EP_KD + KBJ_NU &&
                KBJ_EP_ACTBIAS == KBJ_EP_TAULIM + KBJ_NU && KBJ_EP_JPBIAS == KBJ_EP_ACTBIAS + KBJ_NU && KBJ_EP_MU == KBJ_EP_LATENCY + 1 && KBJ_EP_MU < KBJ_EP_SIZE,
                "the columns of the env parameter row, in the order the word dispatch below walks them");
  __shared__ __align__(16) float p[KBJ_PERT_SIZE];
  const int env = blockIdx.x, lane = threadIdx.x;              // grid = N: env < N
  if (mask && mask[env] == 0.0f) {                             // uniform over the workgroup
    if (status && lane == 0) status[env] = 0;
    return;
  }
  bool ok = true;
  if (lane < KBJ_PERT_SIZE / 4) {
    const float4 v = reinterpret_cast<const float4*>(pert + (size_t)env * KBJ_PERT_SIZE)[lane];
    reinterpret_cast<float4*>(p)[lane] = v;
    ok = pert_word_valid(4 * lane, v.x) && pert_word_valid(4 * lane + 1, v.y) && pert_word_valid(4 * lane + 2, v.z) && pert_word_valid(4 * lane + 3, v.w);
  }
  const bool valid = __all(ok);                                // the workgroup is one wavefront
  if (status && lane == 0) status[env] = valid ? 1 : -1;
  if (!valid) return;                                          // uniform
  __syncthreads();
  float* row = ep + (size_t)env * KBJ_EP_SIZE;
  const int torso = m->torso_body;
  const float* ipos = &m->body_ipos[0][0];
  const float* inertia = &m->body_inertia[0][0];
  const float* cap_pos = &m->cap_pos[0][0];
  for (int k = lane; k <= KBJ_EP_MU; k += 64) {
    float v;
    if (k < KBJ_EP_MASS) v = pert_add(ipos[k], k / 3 == torso ? p[KBJ_PERT_COM_SHIFT + k % 3] : 0.0f);
    else if (k < KBJ_EP_INERTIA) {
      v = pert_mul(m->body_mass[k - KBJ_EP_MASS], p[KBJ_PERT_MASS_SCALE]);
      if (k - KBJ_EP_MASS == torso) v = pert_add(v, p[KBJ_PERT_PAYLOAD]);
    }
    else if (k < KBJ_EP_ARMATURE) v = pert_mul(inertia[k - KBJ_EP_INERTIA], p[KBJ_PERT_MASS_SCALE]);
    else if (k < KBJ_EP_FRICLOSS) v = pert_mul(m->dof_armature[k - KBJ_EP_ARMATURE], p[KBJ_PERT_ARMATURE_SCALE]);
    else if (k < KBJ_EP_CAP_POS) v = pert_mul(m->dof_frictionloss[k - KBJ_EP_FRICLOSS], p[KBJ_PERT_FRICLOSS_SCALE]);
    else if (k < KBJ_EP_CAP_HALF) v = pert_add(cap_pos[k - KBJ_EP_CAP_POS], 0.0f);      // the reset path's own sum with no jitter
    else if (k < KBJ_EP_CAP_RAD) v = m->cap_halflen[k - KBJ_EP_CAP_HALF];
    else if (k < KBJ_EP_KP) v = m->cap_radius[k - KBJ_EP_CAP_RAD];
    else if (k < KBJ_EP_KD) v = pert_mul(m->kp[k - KBJ_EP_KP], p[KBJ_PERT_KP_SCALE + k - KBJ_EP_KP]);
    else if (k < KBJ_EP_TAULIM) v = pert_mul(m->kd[k - KBJ_EP_KD], p[KBJ_PERT_KD_SCALE + k - KBJ_EP_KD]);
    else if (k < KBJ_EP_ACTBIAS) v = pert_mul(m->tau_limit[k - KBJ_EP_TAULIM], p[KBJ_PERT_TAULIM_SCALE + k - KBJ_EP_TAULIM]);
    else if (k < KBJ_EP_JPBIAS) v = p[KBJ_PERT_ACTBIAS + k - KBJ_EP_ACTBIAS];
    else if (k < KBJ_EP_LATENCY) continue;                     // JPBIAS, PGBIAS, PGLAG: the episode's sensor draws stay
    else if (k == KBJ_EP_LATENCY) { if (!(p[KBJ_PERT_LATENCY] >= 0.0f)) continue; v = p[KBJ_PERT_LATENCY]; }
    else v = pert_mul(m->contact_mu, p[KBJ_PERT_MU_SCALE]);
    row[k] = v;
  }
}

// register budget of the step kernel: 13.4 KB of LDS lets 12 single-wavefront workgroups share a CU (3 waves/SIMD), which
// needs <= 168 VGPRs. `amdgpu_num_vgpr(N)` makes hipcc allocate 2 N registers for this wave64 kernel (floor 129): N = 84 gives
// exactly 168 with 61 spilled values. Measured (8192 envs, ms/step): no cap (2 waves/SIMD, no spills) 3.26 -> N = 62 (129 VGPRs,
// 90 spills) 1.98 -> N = 72 (144, 70 spills) 1.83 -> N = 84 (168, 61 spills) 1.80. `amdgpu_waves_per_eu(3,3)` also lands on 168
// registers but schedules worse (2.15).
#ifndef KBJ_ENV_NUM_VGPR
#define KBJ_ENV_NUM_VGPR 84
#endif
// REC: the form that also writes the per-step state record (kbj_traj.qstate_d / kbj_env_record_state). The default rollout runs the other
// one, whose code is exactly the kernel without the feature (two more pointers live through the substep loop cost 2 VGPR / 8 SGPR spills);
// the two are separate __global__ functions so that the hot kernel keeps its name in every profile.
// TERM: the form that also writes the terminal critic row of the envs whose episode ends in this step (kbj_env_step_terminal; task_step's
// critic_term), stamped out the same way: the four kernels without it pass a constant null pointer and carry none of it.
template <bool REC, bool CG, bool TERM = false>
__device__ __forceinline__ void env_step_body(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed,
                                              float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ action,
                                              float* aux_t, float* actor_next, float* critic_next, float* aux_next, int env0, float* qstate_t, float* critic_term = nullptr) {
  __shared__ KbjShared S;
  const int env = env0 + blockIdx.x;   // a launch covers the env range [env0, env0 + gridDim.x)
  PFOR(k, (int)(sizeof(KbjModelLds) / sizeof(float))) reinterpret_cast<float*>(&S.mc)[k] = mc[k];
  PFOR(k, (int)(sizeof(PhysConst) / sizeof(float))) reinterpret_cast<float*>(&S.pc)[k] = reinterpret_cast<const float*>(pcp)[k];
  PFOR(k, KBJ_EP_SIZE) S.ep[k] = ep[(size_t)env * KBJ_EP_SIZE + k];
  PFOR(k, KBJ_ES_SIZE) S.es[k] = es[(size_t)env * KBJ_ES_SIZE + k];
  PFOR(k, 12) S.zrow[k] = 0;
  KBJ_SYNC();
  Rng rng{seed, (uint32_t)(c->env_id_offset + env)};
  const PhysConst& pc = S.pc;
  KBJ_STAMP(18);
  task_step<CG>(S, *m, *c, pc, rng, action + (size_t)env * KBJ_NU, aux_t + (size_t)env * KBJ_AUX_SIZE, actor_next + (size_t)env * KBJ_LD_OF(KBJ_NOBS_ACTOR + c->extra_obs_actor),
            critic_next + (size_t)env * KBJ_LD_OF(KBJ_NOBS_CRITIC + c->extra_obs_critic), aux_next + (size_t)env * KBJ_AUX_SIZE,
            REC ? qstate_t + (size_t)env * KBJ_QSTATE_SIZE : nullptr, TERM ? critic_term + (size_t)env * KBJ_LD_OF(KBJ_NOBS_CRITIC + c->extra_obs_critic) : nullptr);
  if (S.done) PFOR(k, KBJ_EP_SIZE) ep[(size_t)env * KBJ_EP_SIZE + k] = S.ep[k];
  PFOR(k, KBJ_ES_SIZE) es[(size_t)env * KBJ_ES_SIZE + k] = S.es[k];
  KBJ_STAMP(19);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(KBJ_ENV_NUM_VGPR))) void env_step_kernel(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed,
                                                      float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ action,
                                                      float* aux_t, float* actor_next, float* critic_next, float* aux_next, int env0) {
  env_step_body<false, false>(m, c, mc, pcp, seed, ep, es, action, aux_t, actor_next, critic_next, aux_next, env0, nullptr);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(KBJ_ENV_NUM_VGPR))) void env_step_record_kernel(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed,
                                                      float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ action,
                                                      float* aux_t, float* actor_next, float* critic_next, float* aux_next, int env0, float* qstate_t) {
  env_step_body<true, false>(m, c, mc, pcp, seed, ep, es, action, aux_t, actor_next, critic_next, aux_next, env0, qstate_t);
}
// the same two with the Polak-Ribiere CG solver (kbj_config.solver_newton = 0): same register cap, same LDS struct, same launch shape
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(KBJ_ENV_NUM_VGPR))) void env_step_cg_kernel(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed,
                                                      float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ action,
                                                      float* aux_t, float* actor_next, float* critic_next, float* aux_next, int env0) {
  env_step_body<false, true>(m, c, mc, pcp, seed, ep, es, action, aux_t, actor_next, critic_next, aux_next, env0, nullptr);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(KBJ_ENV_NUM_VGPR))) void env_step_record_cg_kernel(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed,
                                                      float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ action,
                                                      float* aux_t, float* actor_next, float* critic_next, float* aux_next, int env0, float* qstate_t) {
  env_step_body<true, true>(m, c, mc, pcp, seed, ep, es, action, aux_t, actor_next, critic_next, aux_next, env0, qstate_t);
}
// the step with the terminal critic rows (kbj_env_step_terminal), both solvers: critic_term [N][ld_critic], rows of envs that go on untouched
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(KBJ_ENV_NUM_VGPR))) void env_step_term_kernel(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed,
                                                      float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ action,
                                                      float* aux_t, float* actor_next, float* critic_next, float* aux_next, int env0, float* critic_term) {
  env_step_body<false, false, true>(m, c, mc, pcp, seed, ep, es, action, aux_t, actor_next, critic_next, aux_next, env0, nullptr, critic_term);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(KBJ_ENV_NUM_VGPR))) void env_step_term_cg_kernel(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ mc, const PhysConst* __restrict__ pcp, uint32_t seed,
                                                      float* __restrict__ ep, float* __restrict__ es, const float* __restrict__ action,
                                                      float* aux_t, float* actor_next, float* critic_next, float* aux_next, int env0, float* critic_term) {
  env_step_body<false, true, true>(m, c, mc, pcp, seed, ep, es, action, aux_t, actor_next, critic_next, aux_next, env0, nullptr, critic_term);
}
// the kernel of the context's solver: NAME_kernel (Newton, the default) or NAME_cg_kernel
#define KBJ_LAUNCH_SOLVER(ctx, NAME, ...) do { \
    if ((ctx)->cfg_h.solver_newton) hipLaunchKernelGGL(NAME##_kernel, __VA_ARGS__); else hipLaunchKernelGGL(NAME##_cg_kernel, __VA_ARGS__); } while (0)

#ifdef KBJ_ENV_STAMPS
extern "C" int kbj_debug_env_stamps(unsigned long long* out32, int clear) {   // diagnostics build only (tools/env_stamps.py)
  if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(kbj_env_stamp_acc), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (clear) { unsigned long long z[32] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(kbj_env_stamp_acc), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
#endif

__global__ void init_reward_carry_kernel(float* carry, int N) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= N) return;
  float* rc = carry + (size_t)env * KBJ_RC_SIZE;
  for (int k = 0; k < KBJ_RC_SIZE; ++k) rc[k] = 0;
  rc[KBJ_RC_CONTACT] = 1.0f; rc[KBJ_RC_CONTACT + 1] = 1.0f;  // train.py:175-178 initial contact carry True
}

}  // namespace

// one control step of all envs on stream s (the kernels' first-env parameter: 0). qstate_t_d: the form with the state record; critic_term_d: the
// form with the terminal critic rows. Both at once is not served (no caller needs it: kbj_rollout and kbj_env_step_terminal refuse it)
int kbj_env_step_all(kbj_ctx* ctx, hipStream_t s, const float* action_d, float* aux_t_d, float* actor_next_d, float* critic_next_d, float* aux_next_d,
                     float* qstate_t_d, float* critic_term_d) {
  if (qstate_t_d && critic_term_d) return kbj_fail(ctx, "env step: the state record and the terminal critic rows cannot be written by one step");
  KbjKernelTimer timer(s, KBJ_KIND_ENV_STEP, 0.0);
  const int N = ctx->cfg_h.num_envs;
  if (critic_term_d)
    KBJ_LAUNCH_SOLVER(ctx, env_step_term, dim3(N), dim3(64), 0, s, ctx->model_d, ctx->cfg_d, ctx->mc_d, (const PhysConst*)ctx->pc_d, ctx->seed, ctx->ep_d, ctx->es_d, action_d, aux_t_d,
                       actor_next_d, critic_next_d, aux_next_d, 0, critic_term_d);
  else if (qstate_t_d)
    KBJ_LAUNCH_SOLVER(ctx, env_step_record, dim3(N), dim3(64), 0, s, ctx->model_d, ctx->cfg_d, ctx->mc_d, (const PhysConst*)ctx->pc_d, ctx->seed, ctx->ep_d, ctx->es_d, action_d, aux_t_d,
                       actor_next_d, critic_next_d, aux_next_d, 0, qstate_t_d);
  else
    KBJ_LAUNCH_SOLVER(ctx, env_step, dim3(N), dim3(64), 0, s, ctx->model_d, ctx->cfg_d, ctx->mc_d, (const PhysConst*)ctx->pc_d, ctx->seed, ctx->ep_d, ctx->es_d, action_d, aux_t_d,
                       actor_next_d, critic_next_d, aux_next_d, 0);
  KBJ_CHECK_LAUNCH(ctx, "env_step_kernel");
  return 0;
}

extern "C" {

int kbj_env_reset_all(kbj_ctx* ctx, uint32_t seed, float* actor0_d, float* critic0_d, float* aux0_d) {
  if (!ctx) return kbj_fail(nullptr, "kbj_env_reset_all: null ctx");
  if (!actor0_d || !critic0_d || !aux0_d) return kbj_fail(ctx, "kbj_env_reset_all: null observation pointer");
  ctx->seed = seed;
  int N = ctx->cfg_h.num_envs;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  hipLaunchKernelGGL(init_reward_carry_kernel, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, ctx->rcarry_d, N);
  KBJ_CHECK_LAUNCH(ctx, "init_reward_carry_kernel");
  KBJ_LAUNCH_SOLVER(ctx, env_reset, dim3(N), dim3(64), 0, ctx->stream, ctx->model_d, ctx->cfg_d, ctx->mc_d, (const PhysConst*)ctx->pc_d, seed, ctx->ep_d, ctx->es_d, actor0_d,
                     critic0_d, aux0_d);
  KBJ_CHECK_LAUNCH(ctx, "env_reset_kernel");
  return 0;
}

int kbj_env_step(kbj_ctx* ctx, const float* action_d, float* aux_t_d, float* actor_next_d, float* critic_next_d, float* aux_next_d) {
  if (!ctx) return kbj_fail(nullptr, "kbj_env_step: null ctx");
  float* q = ctx->qstate_next;
  ctx->qstate_next = nullptr;     // one-shot (kbj_env_record_state), consumed by THIS call whether it succeeds or not: a call that fails early must not
                                  // leave the pointer armed for a later step, when the host may have freed or reused the row
  if (!action_d || !aux_t_d || !actor_next_d || !critic_next_d || !aux_next_d) return kbj_fail(ctx, "kbj_env_step: null pointer");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  return kbj_env_step_all(ctx, ctx->stream, action_d, aux_t_d, actor_next_d, critic_next_d, aux_next_d, q, nullptr);
}

int kbj_env_step_terminal(kbj_ctx* ctx, const float* action_d, float* aux_t_d, float* actor_next_d, float* critic_next_d, float* aux_next_d, float* critic_term_d) {
  if (!ctx) return kbj_fail(nullptr, "kbj_env_step_terminal: null ctx");
  float* q = ctx->qstate_next;
  ctx->qstate_next = nullptr;     // one-shot, consumed by this call as by kbj_env_step
  if (!action_d || !aux_t_d || !actor_next_d || !critic_next_d || !aux_next_d || !critic_term_d) return kbj_fail(ctx, "kbj_env_step_terminal: null pointer");
  if (q) return kbj_fail(ctx, "kbj_env_step_terminal: a state record is armed (kbj_env_record_state); no step kernel writes both the record and the terminal rows - "
                              "record with kbj_env_step, or drop the record");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  return kbj_env_step_all(ctx, ctx->stream, action_d, aux_t_d, actor_next_d, critic_next_d, aux_next_d, nullptr, critic_term_d);
}

int kbj_env_record_state(kbj_ctx* ctx, float* qstate_t_d) {
  if (!ctx) return kbj_fail(nullptr, "kbj_env_record_state: null ctx");
  ctx->qstate_next = qstate_t_d;
  return 0;
}

int kbj_env_reset_where(kbj_ctx* ctx, const float* mask_d, float* actor_next_d, float* critic_next_d, float* aux_next_d) {
  if (!ctx || !mask_d || !actor_next_d || !critic_next_d || !aux_next_d) return kbj_fail(ctx, "kbj_env_reset_where: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  KBJ_LAUNCH_SOLVER(ctx, env_reset_where, dim3(ctx->cfg_h.num_envs), dim3(64), 0, ctx->stream, ctx->model_d, ctx->cfg_d, ctx->mc_d, (const PhysConst*)ctx->pc_d, ctx->seed, ctx->ep_d, ctx->es_d,
                     mask_d, actor_next_d, critic_next_d, aux_next_d);
  KBJ_CHECK_LAUNCH(ctx, "env_reset_where_kernel");
  return 0;
}

int kbj_env_set_command(kbj_ctx* ctx, const float* mask_d, const float* cmd_d, float* actor_next_d, float* critic_next_d, float* aux_next_d) {
  if (!ctx || !cmd_d || !actor_next_d || !critic_next_d || !aux_next_d) return kbj_fail(ctx, "kbj_env_set_command: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  const int N = ctx->cfg_h.num_envs, n = N * KBJ_NCMD;
  hipLaunchKernelGGL(env_set_command_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, N, KBJ_LD_OF(KBJ_NOBS_ACTOR + ctx->cfg_h.extra_obs_actor),
                     KBJ_LD_OF(KBJ_NOBS_CRITIC + ctx->cfg_h.extra_obs_critic), ctx->es_d, mask_d, cmd_d, actor_next_d, critic_next_d, aux_next_d);
  KBJ_CHECK_LAUNCH(ctx, "env_set_command_kernel");
  return 0;
}

int kbj_env_set_push(kbj_ctx* ctx, const float* mask_d, const float* wrench_d, const float* steps_d, const float* next_d) {
  if (!ctx || !wrench_d || !steps_d) return kbj_fail(ctx, "kbj_env_set_push: null argument");
  if (!ctx->cfg_h.enable_pushes) return kbj_fail(ctx, "kbj_env_set_push: this context was created with enable_pushes = 0: its step kernel ignores the push-event state");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  const int N = ctx->cfg_h.num_envs, n = N * 8;
  hipLaunchKernelGGL(env_set_push_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, N, ctx->es_d, mask_d, wrench_d, steps_d, next_d);
  KBJ_CHECK_LAUNCH(ctx, "env_set_push_kernel");
  return 0;
}

int kbj_env_perturb(kbj_ctx* ctx, const float* mask_d, const float* pert_d, int32_t* status_d) {
  if (!ctx || !pert_d) return kbj_fail(ctx, "kbj_env_perturb: null argument");
  if (reinterpret_cast<uintptr_t>(pert_d) & 15) return kbj_fail(ctx, "kbj_env_perturb: pert_d must be 16-byte aligned");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));      // no kbj_nn_drop_prefetch: no observation row is written
  const int N = ctx->cfg_h.num_envs;
  hipLaunchKernelGGL(env_perturb_kernel, dim3(N), dim3(64), 0, ctx->stream, N, ctx->model_d, ctx->ep_d, mask_d, pert_d, status_d);
  KBJ_CHECK_LAUNCH(ctx, "env_perturb_kernel");
  return 0;
}

int kbj_env_get_qstate(kbj_ctx* ctx, float* qpos_d, float* qvel_d) {
  if (!ctx || !qpos_d || !qvel_d) return kbj_fail(ctx, "kbj_env_get_qstate: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  const int N = ctx->cfg_h.num_envs;
  hipLaunchKernelGGL(env_get_qstate_kernel, dim3((N * 64 + 255) / 256), dim3(256), 0, ctx->stream, N, ctx->es_d, qpos_d, qvel_d);
  KBJ_CHECK_LAUNCH(ctx, "env_get_qstate_kernel");
  return 0;
}

int kbj_env_set_qstate(kbj_ctx* ctx, const float* mask_d, const float* qpos_d, const float* qvel_d, float* actor_next_d, float* critic_next_d, float* aux_next_d) {
  if (!ctx || !qpos_d || !qvel_d || !actor_next_d || !critic_next_d || !aux_next_d) return kbj_fail(ctx, "kbj_env_set_qstate: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  KBJ_LAUNCH_SOLVER(ctx, env_set_qstate, dim3(ctx->cfg_h.num_envs), dim3(64), 0, ctx->stream, ctx->model_d, ctx->cfg_d, ctx->mc_d, (const PhysConst*)ctx->pc_d, ctx->seed, ctx->ep_d, ctx->es_d,
                     mask_d, qpos_d, qvel_d, actor_next_d, critic_next_d, aux_next_d);
  KBJ_CHECK_LAUNCH(ctx, "env_set_qstate_kernel");
  return 0;
}

int kbj_env_get_state(kbj_ctx* ctx, float* ep_h, float* es_h) {
  if (!ctx) return kbj_fail(nullptr, "kbj_env_get_state: null ctx");
  size_t N = ctx->cfg_h.num_envs;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  KBJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ep_h) KBJ_HIP(ctx, hipMemcpy(ep_h, ctx->ep_d, N * KBJ_EP_SIZE * sizeof(float), hipMemcpyDeviceToHost));
  if (es_h) KBJ_HIP(ctx, hipMemcpy(es_h, ctx->es_d, N * KBJ_ES_SIZE * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int kbj_env_set_state(kbj_ctx* ctx, const float* ep_h, const float* es_h) {
  if (!ctx) return kbj_fail(nullptr, "kbj_env_set_state: null ctx");
  size_t N = ctx->cfg_h.num_envs;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  KBJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ep_h) KBJ_HIP(ctx, hipMemcpy(ctx->ep_d, ep_h, N * KBJ_EP_SIZE * sizeof(float), hipMemcpyHostToDevice));
  if (es_h) KBJ_HIP(ctx, hipMemcpy(ctx->es_d, es_h, N * KBJ_ES_SIZE * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

int kbj_env_get_reward_carry(kbj_ctx* ctx, float* rc_h) {
  if (!ctx || !rc_h) return kbj_fail(ctx, "kbj_env_get_reward_carry: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  KBJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  KBJ_HIP(ctx, hipMemcpy(rc_h, ctx->rcarry_d, (size_t)ctx->cfg_h.num_envs * KBJ_RC_SIZE * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int kbj_env_set_reward_carry(kbj_ctx* ctx, const float* rc_h) {
  if (!ctx || !rc_h) return kbj_fail(ctx, "kbj_env_set_reward_carry: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  KBJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  KBJ_HIP(ctx, hipMemcpy(ctx->rcarry_d, rc_h, (size_t)ctx->cfg_h.num_envs * KBJ_RC_SIZE * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}


}  // extern "C"
