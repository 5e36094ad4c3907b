// kbj_ctx.h — library context shared by the translation units of libkbj.so (host side only).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <cstdio>
#include "kbj.h"

// per-launch HIP-event records of the MFMA kernels while kbj_profile_begin/end is active (bench.py roofline)
struct KbjKernelRec { int kind; double flops; hipEvent_t a, b; };
enum { KBJ_KIND_GEMM = 0 /* +4 small tile, +2 A k-contiguous, +1 B k-contiguous */, KBJ_KIND_SEQ_FWD = 8, KBJ_KIND_SEQ_BWD = 9, KBJ_KIND_ENV_STEP = 10, KBJ_KIND_SEQ_FWD_FUSED = 11, KBJ_KIND_SEQ_FWD_OBS = 12, KBJ_KIND_LSTM_STEP = 13, KBJ_KIND_LSTM_STEP_OBS = 14,
       // gemm_x3_kernel<TM, A_KC, B_KC, GEN> (kbj_config.gemm_bf16x3), one kind per instantiation the launcher uses: 15..18 = <2, A_KC, B_KC, false>
       // (+2 A k-contiguous, +1 B k-contiguous), 19 = <2, true, true, true>, 20 = <1, true, true, false>, 21 = <1, true, true, true>
       KBJ_KIND_GEMM_X3 = 15, KBJ_KIND_GEMM_X3_GEN = 19, KBJ_KIND_GEMM_X3_SMALL = 20, KBJ_KIND_GEMM_X3_SMALL_GEN = 21,
       KBJ_KIND_SEQ_BWD16 = 22 /* lstm_seq_bwd16_kernel<H> */, KBJ_KIND_GEMM_64x128 = 23 /* gemm_f32_kernel<1, 1, true, true, 2, 4>: the critic's input projection; 24 = <1, 1, true, false, 2, 4>: the input gradients */,
       KBJ_KIND_TRACKING_STATS = 25 /* tracking_stats_kernel (kbj_tracking_stats) */,
       KBJ_KIND_GAIT_STATS = 26 /* gait_stats_kernel (kbj_gait_stats) */,
       KBJ_KIND_ACTUATOR_STATS = 27 /* actuator_stats_kernel (kbj_actuator_stats) */, KBJ_KIND_ACTUATOR_REDUCE = 28 /* its ordered_reduce_wide_kernel<ActSlots> */,
       KBJ_KIND_COUNT = 29 };
inline int kbj_kind_gemm_x3(int tm, bool a_kc, bool b_kc, bool gen) {
  if (tm == 2) return gen ? KBJ_KIND_GEMM_X3_GEN : KBJ_KIND_GEMM_X3 + (a_kc ? 2 : 0) + (b_kc ? 1 : 0);
  return gen ? KBJ_KIND_GEMM_X3_SMALL_GEN : KBJ_KIND_GEMM_X3_SMALL;
}

// Formulation switches of the schedule. A test process builds contexts under different settings; every non-default value below is exercised
// by a parity test (tests/test_gpu_switches.py) and README.md lists exactly these. `deterministic` comes from kbj_config (KBJ_DETERMINISTIC=1
// forces it on).
struct Sched {
  bool fold_actor = true;          // KBJ_FOLD_ACTOR=0: actor input projection as its own GEMM (65 -> H -> 4H) instead of folded into layer 0
  bool fold_critic = true;         // KBJ_FOLD_CRITIC=0: critic layer-0 backward through dX0 instead of Z = dG0^T obs
  bool fuse_ih = true;             // KBJ_SEQ_FUSE=0: input products x W_ih^T as GEMM launches in front of the forward recurrences
  bool fuse_obs = true;            // KBJ_SEQ_FUSE_OBS=0: the folded actor layer 0 as a GEMM launch instead of inside its recurrence
  bool fused_critic_head = true;   // KBJ_FUSED_CRITIC_HEAD=0: critic head as output GEMM + value kernel + loss kernel + K = 1 GEMM
  bool rollout_step = true;        // KBJ_ROLLOUT_STEP=0: rollout layers as [x | h] gate GEMM + cell kernel instead of lstm_step_kernel
  bool one_stream = false;         // KBJ_ONE_STREAM=1: the whole update on the caller's stream (no lanes); forced for wide layers whose two recurrences would not be resident together
  bool debug_sync = false;         // KBJ_DEBUG=1: kbj_ppo_grad synchronises and reports device-side errors at the call that caused them
  bool deterministic = false;      // fixed-order reductions instead of fp32 / fp64 atomics (bit-reproducible update)
  bool bwd16 = true;               // KBJ_BWD16=0: backward recurrences on the 32-row x 32-unit form of rounds 1-4 (lstm_seq_bwd_kernel) instead of 16-row x 64-unit
                                   // tiles with the partner-major contraction (kbj_lstm_bwd16.h: 620 instead of 907 us per launch in situ)
  bool critic_on_caller = true;    // KBJ_CRITIC_LANE=2nd: the critic's chain on the context's SECOND stream (rounds 1-5). Default (round 6): the critic - the longer
                                   // chain, the one a minibatch waits for - runs on the caller's stream, so that nothing between the optimizer step and the
                                   // critic's first kernel, nor between its last kernel and the next optimizer step, crosses a queue (a cross-queue event wait
                                   // costs 10-25 us on this runtime); the actor's chain, which has ~0.3 ms of slack, takes the second stream and the hops.
                                   // kbj_create gives the second stream its queue priority from this same value
  bool gemm_x3 = false;            // kbj_config.gemm_bf16x3 / KBJ_GEMM_X3=1: the GEMM launches that are eligible (the update's input gradients, weight-gradient
                                   // pairs and critic input projection, the rollout's [x | h] gate GEMMs) on the bf16 matrix cores through the exact three-way
                                   // operand split (kbj_gemm.h gemm_x3_kernel); not the default, not the headline
};

struct KbjSettings {
  Sched sched;
  int seq_timeout_ms = 0;          // wall-clock bound of the recurrences' inter-workgroup waits (kbj_lstm_seq.h seq_wait): 2 s by default, KBJ_SEQ_TIMEOUT_MS=n
                                   // (clamped to 1..30000) overrides, 20 ms under fault injection
  // fault injection for the tests (KBJ_DEBUG_DROP_SEQ_WG = n, KBJ_DEBUG_DROP_SEQ_BWD_WG = n): the context's next n forward / backward recurrence
  // launches run with one workgroup missing, so its partners' bounded spins expire and the timeout / fail-stop path is exercised on real
  // hardware. Counted down per affected launch.
  int seq_drop = 0, seq_drop_bwd = 0;
  // diagnostics: per-step clock stamps of one workgroup of one recurrence launch, 1 + net + 2 * layer picks the launch
  bool seq_stamps = false; int stamp_sel = 1;     // KBJ_SEQ_STAMPS (forward)
  bool seq_bstamps = false; int bstamp_sel = 0;   // KBJ_SEQ_BSTAMPS (backward; needs the bstamps build)
};

KbjSettings kbj_read_settings(const kbj_config& cfg);   // kbj_nn.hip

struct kbj_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // second lane for the critic network inside kbj_ppo_grad
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t side[2] = {nullptr, nullptr};   // per-net side lanes for weight-gradient GEMMs
  hipEvent_t ev_dx[2] = {nullptr, nullptr};   // per net lane: the lane's recurrence launches of a layer (the upper layer's weight-gradient pair on the side lane starts behind their END)
  hipEvent_t ev_side[2] = {nullptr, nullptr};
  hipEvent_t ev_obs = nullptr;                // the critic's gathered observation rows are in place (side lane, kbj_nn.hip Update::input_projections)
  hipEvent_t ev_prefetch = nullptr;           // kbj_ppo_prefetch: the next minibatch's head gathers are done
  hipEvent_t ev_small = nullptr;              // the minibatch's small gathers / clears on the actor's side lane are done (kbj_nn.hip Update::gathers)
  hipEvent_t ev_term = nullptr;               // kbj_rollout with kbj_config.gae_terminal_value: the critic lane's terminal-value kernel of a step has read the terminal scratch (RolloutPlan::ev_term)
  hipEvent_t ev_actor_grad = nullptr;         // recorded by kbj_ppo_grad once the ACTOR's slice of the gradient is final (kbj_stream_wait_actor_grad)
  hipEvent_t ev_critic_loss = nullptr;        // kbj_ppo_grad without the fused critic head: the critic lane's loss half is queued (UpdatePlan::ev_critic_loss)
  kbj_model model_h;
  kbj_config cfg_h;
  KbjSettings set;              // the environment's say about this context (kbj_read_settings, once, in kbj_create); the fault-injection counters count down here
  kbj_model* model_d = nullptr;
  kbj_config* cfg_d = nullptr;
  void* pc_d = nullptr;         // kbj::PhysConst (kbj_env_core.h): solver / impedance / terrain constants derived from the config, computed at create
  float* mc_d = nullptr;        // KbjModelLds image (kbj_env_core.h): the model constants every env workgroup copies into LDS
  float* ep_d = nullptr;        // [N][KBJ_EP_SIZE]
  float* es_d = nullptr;        // [N][KBJ_ES_SIZE]
  float* rcarry_d = nullptr;    // [N][KBJ_RC_SIZE] reward carries
  uint32_t seed = 0;
  int rollout_argmax = 0;       // kbj_set_rollout_argmax: kbj_rollout acts with the distribution's mode (validation rollouts, train.py:1564)
  float* qstate_next = nullptr; // kbj_env_record_state: where the next kbj_env_step writes its state record (one-shot)
  double* stats_part_d = nullptr;   // kbj_episode_stats / kbj_tracking_stats / kbj_gait_stats / kbj_actuator_stats: the workgroup partials of the call's scan, stats_part_doubles doubles,
  size_t stats_part_doubles = 0;    // grown by the first call that needs more (kbj_traj_stats.hip stats_partials)
  // NN workspace (kbj_nn.hip)
  void* nn_ws = nullptr;
  size_t nn_ws_bytes = 0;
  // profiling
  bool profiling = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float env_ms = 0, nn_ms = 0;
  int env_launches = 0, nn_launches = 0;
  std::vector<KbjKernelRec> krecs;
  kbj_kernel_stat kstats[KBJ_KIND_COUNT];
  std::string error;
};

// what one translation unit serves to the others
int kbj_nn_create(kbj_ctx* ctx);           // kbj_nn.hip, for kbj_create / kbj_destroy / kbj_synchronize
void kbj_nn_destroy(kbj_ctx* ctx);
int kbj_nn_check_errors(kbj_ctx* ctx);
void kbj_nn_drop_prefetch(kbj_ctx* ctx);   // kbj_nn.hip: a pending next-minibatch hint dies with the trajectory contents it was made from
// kbj_env.hip: one control step of all envs on stream s. qstate_t_d: the form with the state record; critic_term_d: the form with the terminal
// critic rows. Both at once is not served
int kbj_env_step_all(kbj_ctx* ctx, hipStream_t s, const float* action_d, float* aux_t_d, float* actor_next_d, float* critic_next_d, float* aux_next_d,
                     float* qstate_t_d, float* critic_term_d);

extern thread_local std::string kbj_global_error;

inline int kbj_fail(kbj_ctx* ctx, const std::string& msg) {
  if (ctx) ctx->error = msg;
  kbj_global_error = msg;
  return -1;
}

#define KBJ_HIP(ctx, call)                                                                                   \
  do {                                                                                                       \
    hipError_t e_ = (call);                                                                                  \
    if (e_ != hipSuccess) return kbj_fail(ctx, std::string(#call) + ": " + hipGetErrorString(e_));           \
  } while (0)

#define KBJ_CHECK_LAUNCH(ctx, name)                                                                          \
  do {                                                                                                       \
    hipError_t e_ = hipGetLastError();                                                                       \
    if (e_ != hipSuccess) return kbj_fail(ctx, std::string("launch ") + name + ": " + hipGetErrorString(e_)); \
  } while (0)

// the context being profiled on this host thread (nullptr outside kbj_profile_begin/end)
extern thread_local kbj_ctx* kbj_prof_ctx;

// brackets ONE kernel launch on stream s with two timing events
struct KbjKernelTimer {
  kbj_ctx* c; hipStream_t s; hipEvent_t b = nullptr;
  KbjKernelTimer(hipStream_t st, int kind, double flops) : c(kbj_prof_ctx), s(st) {
    if (!c) return;
    hipEvent_t a;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { c = nullptr; return; }
    c->krecs.push_back(KbjKernelRec{kind, flops, a, b});
    hipEventRecord(a, s);
  }
  ~KbjKernelTimer() { if (c) hipEventRecord(b, s); }
};

// timed section helpers for bench.py's roofline (HIP events on the context's stream)
struct KbjTimed {
  kbj_ctx* ctx; bool nn;
  KbjTimed(kbj_ctx* c, bool is_nn) : ctx(c), nn(is_nn) { if (ctx->profiling) hipEventRecord(ctx->ev0, ctx->stream); }
  ~KbjTimed() {
    if (!ctx->profiling) return;
    hipEventRecord(ctx->ev1, ctx->stream);
    hipEventSynchronize(ctx->ev1);
    float ms = 0; hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (nn) { ctx->nn_ms += ms; ctx->nn_launches++; } else { ctx->env_ms += ms; ctx->env_launches++; }
  }
};
