// kbj_traj_stats.hip — HIP kernels + C-ABI entry points of everything that reads a finished trajectory: kbj_rewards (rewards_kernel below),
// kbj_episode_stats (kbj_episode_stats.h), kbj_tracking_stats (kbj_tracking_stats.h), kbj_gait_stats (kbj_gait_stats.h), kbj_push_recovery
// (kbj_push_recovery.h), kbj_step_response (kbj_step_response.h), kbj_frequency_response (kbj_frequency_response.h), kbj_actuator_stats
// (kbj_actuator_stats.h) and kbj_robustness (kbj_robustness.h). None of it is on the hot path, and none of it shares a translation unit with the env kernels (kbj_env.hip): an edit
// here recompiles no step kernel.
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <optional>
#include "kbj_env_core.h"
#include "kbj_ordered_reduce.h"
#include "kbj_episode_stats.h"
#include "kbj_tracking_stats.h"
#include "kbj_gait_stats.h"
#include "kbj_actuator_stats.h"
#include "kbj_ctx.h"
#include "kbj_push_recovery.h"
#include "kbj_step_response.h"
#include "kbj_frequency_response.h"
#include "kbj_robustness.h"

using namespace kbj;

namespace {

// ---- reward stack (train.py:125-506, weights train.py:1225-1256): one thread scans one env's trajectory ----
__global__ void rewards_kernel(const kbj_model* __restrict__ m, const kbj_config* __restrict__ c, const float* __restrict__ aux, int T, int N,
                               float* __restrict__ carry, float* __restrict__ reward, float* __restrict__ comps) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= N) return;
  const float* scales = c->reward_scale;   // user-editable like the reference's get_rewards() (train.py:1224-1256)
  const float ctrl_dt = c->ctrl_dt;
  float* rc = carry + (size_t)env * KBJ_RC_SIZE;
  float tsingle = rc[KBJ_RC_TSINGLE], air[2] = {rc[KBJ_RC_AIRTIME], rc[KBJ_RC_AIRTIME + 1]};
  bool pcon[2] = {rc[KBJ_RC_CONTACT] != 0, rc[KBJ_RC_CONTACT + 1] != 0};
  float pq[6];
  bool pdone = false;
  for (int t = 0; t < T; ++t) {
    const float* a = aux + ((size_t)t * N + env) * KBJ_AUX_SIZE;
    float r[KBJ_NREW];
    const float* cmd = a + KBJ_AUX_CMD;
    bool zc = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1] + cmd[2] * cmd[2]) < 1e-3f;
    bool done = a[KBJ_AUX_DONE] != 0;
    float bq[4] = {a[KBJ_AUX_BQUAT], a[KBJ_AUX_BQUAT + 1], a[KBJ_AUX_BQUAT + 2], a[KBJ_AUX_BQUAT + 3]}, be[3];
    quat_to_euler(bq, be);
    {  // linvel (train.py:274-292)
      float ye[3] = {0, 0, be[2]}, yq[4], v[3] = {cmd[0], cmd[1], 0}, g[3];
      euler_to_quat(ye, yq); rotate_by_quat(v, yq, false, g);
      float ex = a[KBJ_AUX_QVEL] - g[0], ey = a[KBJ_AUX_QVEL + 1] - g[1], err = sqrtf(ex * ex + ey * ey);
      r[KBJ_REW_LINVEL] = expf(-(zc ? err : err * err) / c->rew_linvel_err);
    }
    r[KBJ_REW_ANGVEL] = expf(-fabsf(a[KBJ_AUX_QVEL + 5] - cmd[2]) / c->rew_angvel_err);  // train.py:301-306
    {  // roll_pitch (train.py:316-334)
      float e1[3] = {be[0], be[1], 0}, q1[4], e2[3] = {cmd[4], cmd[5], 0}, q2[4];
      euler_to_quat(e1, q1); euler_to_quat(e2, q2);
      float d_ = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3];
      r[KBJ_REW_ROLL_PITCH] = expf(-(1 - d_ * d_) / (zc ? c->rew_rollpitch_err_zero : c->rew_rollpitch_err));
    }
    {  // base_height (train.py:377-388)
      float low = fminf(a[KBJ_AUX_LFZ] - c->rew_foot_origin_height, a[KBJ_AUX_RFZ] - c->rew_foot_origin_height);
      float h = a[KBJ_AUX_BASEZ] - low;
      r[KBJ_REW_BASE_HEIGHT] = expf(-fabsf(h - (cmd[3] + c->rew_standard_height)) / c->rew_height_err);
    }
    {  // arm_pos (train.py:261-265)
      float e = 0;
      for (int j = 0; j < 10; ++j) { float dq = a[KBJ_AUX_ARMQ + j] - (cmd[6 + j] + m->joint_bias[10 + j]); e += dq * dq; }
      r[KBJ_REW_ARM_POS] = expf(-e / c->rew_armpos_err);
    }
    bool cl = a[KBJ_AUX_TOUCH] > 0.1f, cr = a[KBJ_AUX_TOUCH + 1] > 0.1f;
    {  // single_contact (train.py:138-154), grace period 2.0 s
      float ts = (cl != cr) ? 0.0f : tsingle + ctrl_dt;
      if (zc) ts = c->rew_grace_period;
      tsingle = ts;
      r[KBJ_REW_SINGLE_CONTACT] = zc ? 1.0f : (ts < c->rew_grace_period ? 1.0f : 0.0f);
    }
    r[KBJ_REW_NO_CONTACT] = zc ? 0.0f : ((cl || cr) ? 0.0f : 1.0f);  // train.py:161-165
    {  // feet_airtime (train.py:197-213)
      bool con[2] = {cl, cr};
      float rew = 0;
      for (int f = 0; f < 2; ++f) {
        bool first = con[f] && !pcon[f] && !done;
        rew += (air[f] - c->rew_touchdown_penalty) * (first ? 1.0f : 0.0f);
        air[f] = (con[f] || done) ? 0.0f : air[f] + ctrl_dt;
        pcon[f] = con[f];
      }
      r[KBJ_REW_FEET_AIRTIME] = zc ? 0.0f : rew;
    }
    {  // feet_orient (train.py:418-457)
      float rpy = 0, rp = 0;
      for (int f = 0; f < 2; ++f) {
        const float* fq_ = a + (f ? KBJ_AUX_RFQUAT : KBJ_AUX_LFQUAT);
        float fq[4] = {fq_[0], fq_[1], fq_[2], fq_[3]};
        float te[3] = {f ? 1.5707963267948966f : -1.5707963267948966f, 0, be[2] - 3.141592653589793f}, tq[4];
        euler_to_quat(te, tq);
        float d1 = tq[0] * fq[0] + tq[1] * fq[1] + tq[2] * fq[2] + tq[3] * fq[3];
        rpy += 1 - d1 * d1;
        float fe[3]; quat_to_euler(fq, fe); fe[2] = 0;
        float fq0[4]; euler_to_quat(fe, fq0);
        te[2] = 0; euler_to_quat(te, tq);
        float d2 = tq[0] * fq0[0] + tq[1] * fq0[1] + tq[2] * fq0[2] + tq[3] * fq0[3];
        rp += 1 - d2 * d2;
      }
      r[KBJ_REW_FEET_ORIENT] = expf(-(fabsf(cmd[2]) > 1e-3f ? rp : rpy) / c->rew_feetorient_err);
    }
    {  // com_distance (train.py:466-478)
      float cd = a[KBJ_AUX_COMDIST];
      r[KBJ_REW_COM_DISTANCE] = (cd >= 0 && zc) ? expf(-cd / c->rew_comdist_err) : 0.0f;
    }
    {  // base_accel (train.py:487-494)
      float e = 0;
      if (t > 0 && !pdone) for (int k = 0; k < 6; ++k) e += fabsf(a[KBJ_AUX_QVEL + k] - pq[k]);
      for (int k = 0; k < 6; ++k) pq[k] = a[KBJ_AUX_QVEL + k];
      pdone = done;
      r[KBJ_REW_BASE_ACCEL] = expf(-e / c->rew_baseaccel_err);
    }
    {  // torque (train.py:503-506)
      float s = 0;
      for (int u = 0; u < KBJ_NU; ++u) s += expf(-fabsf(a[KBJ_AUX_CTRL + u]) / c->rew_torque_err);
      r[KBJ_REW_TORQUE] = zc ? s / KBJ_NU : 1.0f;
    }
    float tot = 0;
    for (int k = 0; k < KBJ_NREW; ++k) { tot += scales[k] * r[k]; if (comps) comps[((size_t)t * N + env) * KBJ_NREW + k] = r[k]; }
    reward[(size_t)t * N + env] = tot;
  }
  rc[KBJ_RC_TSINGLE] = tsingle; rc[KBJ_RC_AIRTIME] = air[0]; rc[KBJ_RC_AIRTIME + 1] = air[1];
  rc[KBJ_RC_CONTACT] = pcon[0] ? 1.0f : 0.0f; rc[KBJ_RC_CONTACT + 1] = pcon[1] ? 1.0f : 0.0f;
}

// The workgroup partials of the scans that end in ordered_reduce_kernel: one buffer per context, grown on first use (or for a wider
// trajectory than any before), never per call. The scans run on the context's stream, so a call's reduce has read the partials before the
// next call's scan writes them; the hipFree of a growth synchronises the device.
int stats_partials(kbj_ctx* ctx, size_t doubles) {
  if (doubles <= ctx->stats_part_doubles) return 0;
  if (ctx->stats_part_d) KBJ_HIP(ctx, hipFree(ctx->stats_part_d));
  ctx->stats_part_d = nullptr; ctx->stats_part_doubles = 0;
  KBJ_HIP(ctx, hipMalloc(&ctx->stats_part_d, doubles * sizeof(double)));
  ctx->stats_part_doubles = doubles;
  return 0;
}

// "<fn>: the trajectory needs <its arrays> and positive T, N"
int check_traj(kbj_ctx* ctx, const char* fn, const kbj_traj* tr, bool needs_reward) {
  if (tr->aux_d && (!needs_reward || tr->reward_d) && tr->T > 0 && tr->N > 0) return 0;
  return kbj_fail(ctx, std::string(fn) + ": the trajectory needs " + (needs_reward ? "aux_d, reward_d" : "aux_d") + " and positive T, N");
}

// "<fn>: <names> must be 16-byte aligned" (a null pointer is aligned)
int check_aligned16(kbj_ctx* ctx, const char* fn, const char* names, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15) ? kbj_fail(ctx, std::string(fn) + ": " + names + " must be 16-byte aligned") : 0;
}

// a scan that leaves `blocks` workgroup partials of Slots::SIZE doubles, then their ordered reduce into stats_d: the wide one where a vector
// is wider than one workgroup. launch_scan(partials) queues the scan on the context's stream; reduce_kind >= 0 times the reduce as that kind
template <class Slots, class LaunchScan>
int scan_then_reduce(kbj_ctx* ctx, int blocks, const char* scan_name, const char* reduce_name, double* stats_d, LaunchScan launch_scan, int reduce_kind = -1) {
  if (stats_partials(ctx, (size_t)blocks * Slots::SIZE) != 0) return -1;
  launch_scan(ctx->stats_part_d);
  KBJ_CHECK_LAUNCH(ctx, scan_name);
  {
    std::optional<KbjKernelTimer> timer;
    if (reduce_kind >= 0) timer.emplace(ctx->stream, reduce_kind, 0.0);
    if constexpr (Slots::SIZE > ORDERED_REDUCE_THREADS)
      hipLaunchKernelGGL(ordered_reduce_wide_kernel<Slots>, dim3(Slots::SIZE / ORDERED_REDUCE_THREADS), dim3(ORDERED_REDUCE_THREADS), 0, ctx->stream, ctx->stats_part_d, blocks, stats_d);
    else
      hipLaunchKernelGGL(ordered_reduce_kernel<Slots>, dim3(1), dim3(ORDERED_REDUCE_THREADS), 0, ctx->stream, ctx->stats_part_d, blocks, stats_d);
  }
  KBJ_CHECK_LAUNCH(ctx, reduce_name);
  return 0;
}

// "<fn>: G must be in [1, 256]", where the group statistics are asked for
int check_groups(kbj_ctx* ctx, const char* fn, int G, const double* stats_d) {
  return (stats_d && (G < 1 || G > GROUP_REDUCE_THREADS)) ? kbj_fail(ctx, std::string(fn) + ": G must be in [1, 256]") : 0;
}

// a window scan over ceil(N / WINDOW_ENVS) workgroups of one wavefront - launch_scan(grid, block) queues it on the context's stream - then,
// when stats_d is given, its group reduce: rec_d [N] by group_d into stats_d [G]
template <class Rec, class LaunchScan>
int window_scan_then_reduce(kbj_ctx* ctx, int N, const char* scan_name, LaunchScan launch_scan, void (*reduce)(const Rec*, const int32_t*, int, int, double*),
                            const char* reduce_name, const Rec* rec_d, const int32_t* group_d, int G, double* stats_d) {
  launch_scan(dim3((N + WINDOW_ENVS - 1) / WINDOW_ENVS), dim3(WINDOW_ENVS));
  KBJ_CHECK_LAUNCH(ctx, scan_name);
  if (stats_d) {
    hipLaunchKernelGGL(reduce, dim3(1), dim3(GROUP_REDUCE_THREADS), 0, ctx->stream, rec_d, group_d, N, G, stats_d);
    KBJ_CHECK_LAUNCH(ctx, reduce_name);
  }
  return 0;
}

// stage 1 of kbj_step_response and kbj_frequency_response: the signal of rows 0 .. T-1 of the trajectory's aux rows into sig_d
int launch_step_signal(kbj_ctx* ctx, const kbj_traj* tr, float* sig_d) {
  const size_t rows = (size_t)tr->T * (size_t)tr->N;
  const size_t sig_blocks = (rows + SR_SIG_THREADS - 1) / SR_SIG_THREADS;
  hipLaunchKernelGGL(step_signal_kernel, dim3((unsigned)(sig_blocks < (1u << 20) ? sig_blocks : (1u << 20))), dim3(SR_SIG_THREADS), 0, ctx->stream, tr->aux_d, rows, sig_d);
  KBJ_CHECK_LAUNCH(ctx, "step_signal_kernel");
  return 0;
}

}  // namespace

extern "C" {

int kbj_rewards(kbj_ctx* ctx, const float* aux_d, int T, float* reward_d, float* comps_d) {
  if (!ctx) return kbj_fail(nullptr, "kbj_rewards: null ctx");
  if (!aux_d || !reward_d || T <= 0) return kbj_fail(ctx, "kbj_rewards: bad arguments");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  int N = ctx->cfg_h.num_envs;
  hipLaunchKernelGGL(rewards_kernel, dim3((N + 63) / 64), dim3(64), 0, ctx->stream, ctx->model_d, ctx->cfg_d, aux_d, T, N, ctx->rcarry_d,
                     reward_d, comps_d);
  KBJ_CHECK_LAUNCH(ctx, "rewards_kernel");
  return 0;
}

int kbj_episode_stats(kbj_ctx* ctx, const kbj_traj* tr, float* acc_d, double* stats_d) {
  if (!ctx || !tr || !acc_d || !stats_d) return kbj_fail(ctx, "kbj_episode_stats: null argument");
  if (check_traj(ctx, "kbj_episode_stats", tr, true) != 0 || check_aligned16(ctx, "kbj_episode_stats", "acc_d and reward_comps_d", {acc_d, tr->reward_comps_d}) != 0) return -1;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  const int blocks = (tr->N + EPST_ENVS - 1) / EPST_ENVS;
  return scan_then_reduce<EpstSlots>(ctx, blocks, "episode_stats_kernel", "ordered_reduce_kernel<EpstSlots>", stats_d, [&](double* part_d) {
    hipLaunchKernelGGL(episode_stats_kernel, dim3(blocks), dim3(EPST_THREADS), 0, ctx->stream, tr->aux_d, tr->reward_d, tr->reward_comps_d, tr->T, tr->N,
                       ctx->cfg_h.unhealthy_z, acc_d, part_d);
  });
}

int kbj_tracking_stats(kbj_ctx* ctx, const kbj_traj* tr, int settle_steps, float* acc_d, double* stats_d, float* err_d) {
  if (!ctx || !tr || !acc_d || !stats_d) return kbj_fail(ctx, "kbj_tracking_stats: null argument");
  if (check_traj(ctx, "kbj_tracking_stats", tr, false) != 0) return -1;
  if (settle_steps < 0) return kbj_fail(ctx, "kbj_tracking_stats: settle_steps must not be negative");
  if (check_aligned16(ctx, "kbj_tracking_stats", "acc_d, err_d and aux_d", {acc_d, err_d, tr->aux_d}) != 0) return -1;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  kbj_nn_drop_prefetch(ctx);
  const int blocks = (tr->N + TRK_ENVS - 1) / TRK_ENVS;
  return scan_then_reduce<TrkSlots>(ctx, blocks, "tracking_stats_kernel", "ordered_reduce_kernel<TrkSlots>", stats_d, [&](double* part_d) {
    KbjKernelTimer timer(ctx->stream, KBJ_KIND_TRACKING_STATS, 0.0);
    hipLaunchKernelGGL(tracking_stats_kernel, dim3(blocks), dim3(TRK_THREADS), 0, ctx->stream, ctx->model_d, tr->aux_d, tr->T, tr->N, settle_steps,
                       ctx->cfg_h.rew_standard_height, ctx->cfg_h.rew_foot_origin_height, acc_d, part_d, err_d);
  });
}

int kbj_gait_stats(kbj_ctx* ctx, const kbj_traj* tr, float* acc_d, double* stats_d, float* env_d) {
  if (!ctx || !tr || !acc_d || !stats_d) return kbj_fail(ctx, "kbj_gait_stats: null argument");
  if (check_traj(ctx, "kbj_gait_stats", tr, false) != 0 || check_aligned16(ctx, "kbj_gait_stats", "acc_d, env_d and aux_d", {acc_d, env_d, tr->aux_d}) != 0) return -1;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));      // no kbj_nn_drop_prefetch: no trajectory row is written
  const int blocks = (tr->N + GAIT_ENVS - 1) / GAIT_ENVS;
  return scan_then_reduce<GaitSlots>(ctx, blocks, "gait_stats_kernel", "ordered_reduce_kernel<GaitSlots>", stats_d, [&](double* part_d) {
    KbjKernelTimer timer(ctx->stream, KBJ_KIND_GAIT_STATS, 0.0);
    hipLaunchKernelGGL(gait_stats_kernel, dim3(blocks), dim3(GAIT_THREADS), 0, ctx->stream, tr->aux_d, tr->T, tr->N, acc_d, part_d, env_d);
  });
}

int kbj_actuator_stats(kbj_ctx* ctx, const kbj_traj* tr, const kbj_actuator_levels* lv, float* acc_d, double* stats_d, float* env_d) {
  if (!ctx || !tr || !lv || !acc_d || !stats_d) return kbj_fail(ctx, "kbj_actuator_stats: null argument");
  if (!tr->qstate_d) return kbj_fail(ctx, "kbj_actuator_stats: the trajectory has no qstate_d: joint positions and speeds come from the state record (kbj_env_record_state; HumanoidWalkingTaskConfig.record_state)");
  if (!tr->aux_d || !tr->action_d || tr->T <= 0 || tr->N <= 0) return kbj_fail(ctx, "kbj_actuator_stats: the trajectory needs aux_d, action_d, qstate_d and positive T, N");
  if (check_aligned16(ctx, "kbj_actuator_stats", "acc_d, env_d, aux_d, action_d and qstate_d", {acc_d, env_d, tr->aux_d, tr->action_d, tr->qstate_d}) != 0) return -1;
  for (int u = 0; u < KBJ_NU; ++u) {
    if (!(lv->tau_level[u] > 0.0f)) return kbj_fail(ctx, "kbj_actuator_stats: a tau_level is not positive or NaN");
    if (!(lv->vel_level[u] > 0.0f)) return kbj_fail(ctx, "kbj_actuator_stats: a vel_level is not positive or NaN (+inf counts nothing)");
    if (!(lv->pos_lo[u] <= lv->pos_hi[u])) return kbj_fail(ctx, "kbj_actuator_stats: pos_lo > pos_hi, or one of them is NaN");
  }
  KBJ_HIP(ctx, hipSetDevice(ctx->device));      // no kbj_nn_drop_prefetch: no trajectory row is written
  const int blocks = (tr->N + ACT_ENVS - 1) / ACT_ENVS;
  return scan_then_reduce<ActSlots>(ctx, blocks, "actuator_stats_kernel", "ordered_reduce_wide_kernel<ActSlots>", stats_d, [&](double* part_d) {
    KbjKernelTimer timer(ctx->stream, KBJ_KIND_ACTUATOR_STATS, 0.0);
    hipLaunchKernelGGL(actuator_stats_kernel, dim3(blocks), dim3(ACT_THREADS), 0, ctx->stream, tr->aux_d, tr->qstate_d, tr->action_d, tr->T, tr->N, *lv, acc_d, part_d, env_d);
  }, KBJ_KIND_ACTUATOR_REDUCE);
}

int kbj_push_recovery(kbj_ctx* ctx, const kbj_traj* tr, const float* err_d, const int32_t* sched_d, const kbj_push_criteria* crit, float* rec_d,
                      const int32_t* group_d, int G, double* stats_d) {
  if (!ctx || !tr || !err_d || !sched_d || !crit || !rec_d) return kbj_fail(ctx, "kbj_push_recovery: null argument");
  if (check_traj(ctx, "kbj_push_recovery", tr, false) != 0 || check_aligned16(ctx, "kbj_push_recovery", "err_d and rec_d", {err_d, rec_d}) != 0) return -1;
  if (reinterpret_cast<uintptr_t>(sched_d) & 7) return kbj_fail(ctx, "kbj_push_recovery: sched_d must be 8-byte aligned");
  if (crit->hold_steps < 1) return kbj_fail(ctx, "kbj_push_recovery: hold_steps must be at least 1");
  if (crit->window_steps < 0) return kbj_fail(ctx, "kbj_push_recovery: window_steps must not be negative");
  for (int k = 0; k < KBJ_NTERR; ++k)
    if (crit->tol[k] != crit->tol[k]) return kbj_fail(ctx, "kbj_push_recovery: a tolerance is NaN (+inf ignores a column)");
  if (check_groups(ctx, "kbj_push_recovery", G, stats_d) != 0) return -1;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  return window_scan_then_reduce<float>(ctx, tr->N, "push_recovery_kernel", [&](dim3 grid, dim3 block) {
    hipLaunchKernelGGL(push_recovery_kernel, grid, block, 0, ctx->stream, err_d, tr->aux_d, tr->T, tr->N, sched_d, *crit, rec_d);
  }, push_recovery_reduce_kernel, "push_recovery_reduce_kernel", rec_d, group_d, G, stats_d);
}

int kbj_step_response(kbj_ctx* ctx, const kbj_traj* tr, const int32_t* sched_d, const kbj_step_criteria* crit, float* sig_d, float* rec_d,
                      const int32_t* group_d, int G, double* stats_d) {
  if (!ctx || !tr || !sched_d || !crit || !sig_d || !rec_d) return kbj_fail(ctx, "kbj_step_response: null argument");
  if (check_traj(ctx, "kbj_step_response", tr, false) != 0 || check_aligned16(ctx, "kbj_step_response", "aux_d, sig_d and rec_d", {tr->aux_d, sig_d, rec_d}) != 0) return -1;
  if (crit->smooth_steps < 1 || crit->smooth_steps > SR_RING) return kbj_fail(ctx, "kbj_step_response: smooth_steps must be in [1, 32]");
  static_assert(SR_RING == 32, "the smooth_steps range kbj.h documents");
  if (crit->hold_steps < 1) return kbj_fail(ctx, "kbj_step_response: hold_steps must be at least 1");
  if (crit->window_steps < 1) return kbj_fail(ctx, "kbj_step_response: window_steps must be at least 1");
  if (!(crit->rise_level > 0.0f && crit->rise_level <= 1.0f)) return kbj_fail(ctx, "kbj_step_response: rise_level must be in (0, 1]");
  if (!(crit->band_frac >= 0.0f)) return kbj_fail(ctx, "kbj_step_response: band_frac is negative or NaN");
  for (int k = 0; k < KBJ_NSCH; ++k) {
    if (!(crit->band_abs[k] >= 0.0f)) return kbj_fail(ctx, "kbj_step_response: a band_abs is negative or NaN");
    if (!(crit->min_step[k] >= 0.0f)) return kbj_fail(ctx, "kbj_step_response: a min_step is negative or NaN");
  }
  if (check_groups(ctx, "kbj_step_response", G, stats_d) != 0) return -1;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));      // no kbj_nn_drop_prefetch: no trajectory row is written
  if (launch_step_signal(ctx, tr, sig_d) != 0) return -1;
  return window_scan_then_reduce<float>(ctx, tr->N, "step_scan_kernel", [&](dim3 grid, dim3 block) {
    hipLaunchKernelGGL(step_scan_kernel, grid, block, 0, ctx->stream, sig_d, tr->T, tr->N, sched_d, *crit, rec_d);
  }, step_reduce_kernel, "step_reduce_kernel", rec_d, group_d, G, stats_d);
}

int kbj_frequency_response(kbj_ctx* ctx, const kbj_traj* tr, const int32_t* sched_d, const kbj_frequency_criteria* crit, float* sig_d, double* rec_d,
                           const int32_t* group_d, int G, double* stats_d) {
  if (!ctx || !tr || !sched_d || !crit || !sig_d || !rec_d) return kbj_fail(ctx, "kbj_frequency_response: null argument");
  if (check_traj(ctx, "kbj_frequency_response", tr, false) != 0 || check_aligned16(ctx, "kbj_frequency_response", "aux_d, sig_d and sched_d", {tr->aux_d, sig_d, sched_d}) != 0) return -1;
  if ((reinterpret_cast<uintptr_t>(rec_d) | reinterpret_cast<uintptr_t>(stats_d)) & 7) return kbj_fail(ctx, "kbj_frequency_response: rec_d and stats_d must be 8-byte aligned");
  for (int k = 0; k < KBJ_NSCH; ++k)
    if (!(crit->min_amp[k] >= 0.0f)) return kbj_fail(ctx, "kbj_frequency_response: a min_amp is negative or NaN");
  if (check_groups(ctx, "kbj_frequency_response", G, stats_d) != 0) return -1;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));      // no kbj_nn_drop_prefetch: no trajectory row is written
  if (launch_step_signal(ctx, tr, sig_d) != 0) return -1;
  return window_scan_then_reduce<double>(ctx, tr->N, "freq_scan_kernel", [&](dim3 grid, dim3 block) {
    hipLaunchKernelGGL(freq_scan_kernel, grid, block, 0, ctx->stream, sig_d, tr->T, tr->N, sched_d, *crit, rec_d);
  }, freq_reduce_kernel, "freq_reduce_kernel", rec_d, group_d, G, stats_d);
}

int kbj_robustness(kbj_ctx* ctx, const kbj_traj* tr, const float* err_d, double* rec_d, const int32_t* group_d, int G, double* stats_d) {
  if (!ctx || !tr || !err_d || !rec_d) return kbj_fail(ctx, "kbj_robustness: null argument");
  if (check_traj(ctx, "kbj_robustness", tr, false) != 0 || check_aligned16(ctx, "kbj_robustness", "err_d and rec_d", {err_d, rec_d}) != 0) return -1;
  if (check_groups(ctx, "kbj_robustness", G, stats_d) != 0) return -1;
  KBJ_HIP(ctx, hipSetDevice(ctx->device));      // no kbj_nn_drop_prefetch: no trajectory row is written
  return window_scan_then_reduce<double>(ctx, tr->N, "robustness_scan_kernel", [&](dim3 grid, dim3 block) {
    hipLaunchKernelGGL(robustness_scan_kernel, grid, block, 0, ctx->stream, err_d, tr->aux_d, tr->T, tr->N, rec_d);
  }, robustness_reduce_kernel, "robustness_reduce_kernel", rec_d, group_d, G, stats_d);
}

}  // extern "C"
