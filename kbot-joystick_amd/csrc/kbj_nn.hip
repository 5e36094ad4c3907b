// kbj_nn.hip — LSTM actor-critic + PPO update on the GPU (C ABI: kbj_policy_step, kbj_rollout, kbj_gae, kbj_ppo_grad,
// kbj_adamw_step, kbj_init_params). SURVEY.md §8 rows a4-a13. All matrix products run on the fp32 matrix cores
// (kbj_gemm.h); activations needed by back-propagation-through-time are stashed in HBM (sized for 288 GB).
#include <hip/hip_runtime.h>
#include <vector>
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <type_traits>
#include "kbj_ctx.h"
#include "kbj_gemm.h"
#include "kbj_nn_kernels.h"
#include "kbj_lstm_seq.h"
#include "kbj_lstm_bwd16.h"
#include "kbj_deploy.h"
#include "kbj_terminal_value.h"

using namespace kbj;

namespace {

constexpr int MAXD = KBJ_MAX_DEPTH;   // LSTM layers per net (config.depth = 1..MAXD; train.py:82-85 default 2)

struct NetOff {  // float offsets into the flat parameter vector (kbj.h layout = equinox leaf order)
  size_t w_in, b_in, w_ih[MAXD], w_hh[MAXD], b[MAXD], w_out, b_out;
  int nin, nout, ld_obs;
};

struct TrainBufs {  // per net, minibatch-sized
  float *obs, *X0, *G[MAXD], *Hm[MAXD], *Hout[MAXD], *Cm[MAXD], *TanhC[MAXD], *Out, *dOut, *dHa, *dHb, *dGl[MAXD];
};

// where every leaf sits in the flat parameter vector of a given hidden size
struct ParamLayout {
  NetOff net[2];
  size_t nparams = 0, nactor = 0;
  int D = 2;
};

struct NnWs : ParamLayout {   // (the base: the layout at the kernels' H)
  Sched& sched;               // the context's (kbj_ctx::set)
  explicit NnWs(Sched& s) : sched(s) {}
  int H = 0, N = 0, B = 0, T = 0;
  // hidden_size is free (train.py:78-81); the kernels tile hidden units in groups of 64. Hu = the caller's value, H = the kernels'.
  // Hu != H: every entry point that takes parameters, carries or a gradient converts at the boundary (zero padding is exact for this
  // network: a padded unit has zero weights and bias, so its gates are sigma(0), tanh(0), its cell stays 0, its output 0, and every
  // gradient into or out of it is 0) and runs the H-wide schedule on the internal copies below.
  int Hu = 0;
  ParamLayout user;                   // the caller's layout (Hu)
  PadDesc* pad_desc = nullptr; int npad = 0;
  float *pparams = nullptr, *pgrad = nullptr;
  float *phc[4] = {nullptr, nullptr, nullptr, nullptr}, *pc0[4] = {nullptr, nullptr, nullptr, nullptr};   // carries / trajectory start carries [D][2][N][H]
  bool padded() const { return Hu != H; }
  // deterministic mode: per-lane workspaces (lane = stream: caller's, second, side 0, side 1) for split-K slabs and reduction partials
  float* skws[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t skws_cap[4] = {0, 0, 0, 0};
  float* detp[4] = {nullptr, nullptr, nullptr, nullptr};   // [512][1024] floats each
  double* detd = nullptr;                                    // [512][2] doubles (advantage statistics, gradient norm)
  // rollout scratch
  float *rX[4] = {nullptr, nullptr, nullptr, nullptr}, *rG[4] = {nullptr, nullptr, nullptr, nullptr}, *rOut[4] = {nullptr, nullptr, nullptr, nullptr};
  float* joint_bias_d = nullptr;
  // mirror aux losses (nets 2, 3 = actor, critic evaluated on mirrored observations with the SAME weights)
  bool mirror = false;
  int nnets = 2;
  MirrorEntry* mtab[2] = {nullptr, nullptr};
  float *rObsM[2] = {nullptr, nullptr};   // rollout: mirrored observation rows [N][ld]
  float* rH[4][MAXD] = {};                  // rollout: the h planes' ping-pong partners [N][H] per (net, layer)
  float* tail_hc = nullptr;                 // kbj_config.gae_tail_value: the critic carry copy [D][2][N][H] that kbj_critic_value / the rollout's tail pass steps instead of the caller's
  // kbj_config.gae_terminal_value: the env step's terminal critic rows [N][ld_critic] (allocated with the switch on only) and the caller's
  // [T][N] buffer of their values (kbj_set_terminal_values: kbj_rollout writes it, kbj_gae reads it)
  float *term_rows = nullptr, *value_term = nullptr;
  float *y_m = nullptr, *sd_m = nullptr, *value_m = nullptr, *lpf0_m = nullptr, *dy = nullptr, *dy_m = nullptr, *dvalue_m = nullptr, *zeroR = nullptr;
  // training
  TrainBufs tb[4];
  float *keep = nullptr, *act = nullptr, *logp_old = nullptr, *val_old = nullptr, *adv = nullptr, *target = nullptr;
  float *y = nullptr, *sd = nullptr, *logp = nullptr, *ent = nullptr, *value = nullptr, *dlogp = nullptr, *dvalue = nullptr, *lpf0 = nullptr;
  // actor layer 0 with the input projection folded in (the projection has no activation and 65 < H inputs):
  // W_eff = W_ih0 W_in [4H][68 (65 used)], b_eff = W_ih0 b_in + b_0; Zeff[n] = dG0^T obs of actor-type net n (n = 0, 2)
  float *Weff = nullptr, *beff = nullptr, *Zeff[4] = {nullptr, nullptr, nullptr, nullptr};
  float* WinP[2] = {nullptr, nullptr};   // input-projection weights re-pitched to the observation rows' 16-byte aligned stride (per call: the parameters change)
  double* stats = nullptr;  // [0..1] adv stats, [2..9] metric accumulators, [10] grad sumsq, [11] sample count of caller-supplied adv sums (0: own minibatch)
  const int32_t* prefetched_idx = nullptr;   // kbj_ppo_prefetch: the gathers of the next kbj_ppo_grad / kbj_ppo_forward with these indices are already queued
  const kbj_traj* prefetched_traj = nullptr;
  const double* ext_adv_sums = nullptr;   // kbj_set_advantage_sums: (sum adv, sum adv^2, count) on the device, used instead of the minibatch's own statistics
  unsigned* seq_counters = nullptr;  // per row-group arrival counters of the persistent LSTM kernels
  unsigned* seq_err = nullptr;       // spin-timeout flag
  unsigned seq_timeout_ticks = 0;    // KbjSettings::seq_timeout_ms in wall_clock64 ticks of this device
  bool counters_clean = false;       // the hand-off counters were cleared at the tail of the last kbj_ppo_grad (per lane, behind its last recurrence): the next call skips its own clear
  bool sumsq_clean = false;          // stats[10] (the gradient's sum of squares) has been zeroed by kbj_ppo_grad's own clear and not used since: kbj_adamw_step skips its memset
  int seq_grid = 0, seq_slots = 0;   // workgroups of one recurrence launch / resident workgroups of the worst-fitting recurrence kernel (kbj_recurrence_residency)
  long long* seq_stamps = nullptr;   // diagnostics (KBJ_SEQ_STAMPS=1): per-step clock stamps of one workgroup
  long long* seq_bstamps = nullptr;  // same for a backward recurrence (KBJ_SEQ_BSTAMPS = 1 + net + 2 * layer)
  std::vector<void*> allocs;
};

NnWs* ws_of(kbj_ctx* ctx) { return reinterpret_cast<NnWs*>(ctx->nn_ws); }

ParamLayout layout_params(const kbj_config& c, int H) {
  ParamLayout p;
  const int D = p.D = c.depth;
  size_t off = 0;
  for (int n = 0; n < 2; ++n) {
    NetOff& o = p.net[n];
    o.nin = n == 0 ? KBJ_NOBS_ACTOR + c.extra_obs_actor : KBJ_NOBS_CRITIC + c.extra_obs_critic;     // user observation columns behind the reference's (kbj_model.h)
    o.ld_obs = KBJ_LD_OF(o.nin);
    o.nout = n == 0 ? 2 * KBJ_NU : 1;
    o.w_in = off; off += (size_t)H * o.nin;
    o.b_in = off; off += H;
    for (int l = 0; l < D; ++l) {
      o.w_ih[l] = off; off += (size_t)4 * H * H;
      o.w_hh[l] = off; off += (size_t)4 * H * H;
      o.b[l] = off; off += (size_t)4 * H;
    }
    o.w_out = off; off += (size_t)o.nout * H;
    o.b_out = off; off += o.nout;
    if (n == 0) p.nactor = off;
  }
  p.nparams = off;
  return p;
}

// the carries of net n (0 actor, 1 critic, 2 / 3 their mirror branches) in a kbj_carry, the start carries in a kbj_traj
template <class C> auto& carry_hc(C& c, int n) { return n == 0 ? c.actor_hc_d : n == 1 ? c.critic_hc_d : n == 2 ? c.actor_mirror_hc_d : c.critic_mirror_hc_d; }
template <class T> auto& traj_carry0(T& t, int n) { return n == 0 ? t.carry0_actor_hc_d : n == 1 ? t.carry0_critic_hc_d : n == 2 ? t.carry0_actor_mirror_hc_d : t.carry0_critic_mirror_hc_d; }
// the mirror losses are on and this carry / this trajectory (null: not part of the call) lacks one of the mirror-branch arrays
bool mirror_arrays_missing(bool mirror, const kbj_carry* c, const kbj_traj* t) {
  return mirror && ((c && (!c->actor_mirror_hc_d || !c->critic_mirror_hc_d || !c->lpf_mirror_d)) ||
                    (t && (!t->carry0_actor_mirror_hc_d || !t->carry0_critic_mirror_hc_d || !t->carry0_lpf_mirror_d)));
}

// build_mirror_tables (the (source index, multiplier, offset) tables of mirror_rows_kernel): kbj_nn_kernels.h, beside the kernel

template <class T> int dalloc(kbj_ctx* ctx, NnWs& w, T** p, size_t count) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, count * sizeof(T));
  if (e != hipSuccess) return kbj_fail(ctx, std::string("hipMalloc (nn workspace): ") + hipGetErrorString(e));
  w.allocs.push_back(q);
  *p = reinterpret_cast<T*>(q);
  return 0;
}

constexpr int g_fold_sk = 8;        // k slices of the small W_ih0^T Z product of the folded input projections
#ifndef KBJ_SPLITK_WGS
#define KBJ_SPLITK_WGS 768   // re-swept in round 5 under the four-launches-together schedule: 256 / 384 / 512 / 768 / 1024 -> 6.10 / 6.0 / 5.96 / 5.86 / 5.95 ms per minibatch
#endif
constexpr int g_splitk_wgs = KBJ_SPLITK_WGS;   // target number of workgroups of a split-K weight-gradient GEMM (512 ... 1536 measured flat)
constexpr int DETP_COLS = 4 * 512;   // (rows: DETP_ROWS, kbj_nn_kernels.h; columns: one gate row of the widest layer, 4 SEQ_MAX_H)

// lane index of a stream of this context (deterministic-mode workspaces are per lane: launches on different lanes overlap)
int lane_of(kbj_ctx* ctx, hipStream_t s) { return s == ctx->stream ? 0 : (s == ctx->stream2 ? 1 : (s == ctx->side[0] ? 2 : 3)); }
// split-K slab workspace of the lane of stream s, grown on demand (deterministic mode only; null otherwise = atomics)
float* sk_workspace(kbj_ctx* ctx, hipStream_t s, size_t floats) {
  NnWs& w = *ws_of(ctx);
  if (!w.sched.deterministic) return nullptr;
  const int l = lane_of(ctx, s);
  if (w.skws_cap[l] < floats) {   // grows during the first calls only; nothing may still be reading the old slab
    hipDeviceSynchronize();
    if (w.skws[l]) hipFree(w.skws[l]);
    w.skws[l] = nullptr; w.skws_cap[l] = 0;
    void* q = nullptr;
    if (hipMalloc(&q, floats * sizeof(float)) != hipSuccess) { kbj_fail(ctx, "hipMalloc (deterministic split-K workspace)"); return nullptr; }
    w.skws[l] = reinterpret_cast<float*>(q); w.skws_cap[l] = floats;
  }
  return w.skws[l];
}
float* det_partials(kbj_ctx* ctx, hipStream_t s) {
  NnWs& w = *ws_of(ctx);
  return w.sched.deterministic ? w.detp[lane_of(ctx, s)] : nullptr;
}

// y = x W^T + b  (x [M][K] lda, W [N][K])
void linear_fwd(hipStream_t s, const float* x, int lda, const float* W, int ldw, const float* bias, float* y, int ldy, int M, int N, int K, int beta) {
  GemmArgs g{x, W, y, bias, M, N, K, lda, ldw, ldy, beta, 1, nullptr};
  gemm_launch<true, true>(s, g);
}
// dx = dy W   (dy [M][K=nout] , W [K][N]). x3 here and below: the caller's Sched::gemm_x3
void linear_bwd_input(hipStream_t s, bool x3, const float* dy, int lddy, const float* W, int ldw, float* dx, int lddx, int M, int N, int K, int beta, int tile = -1) {
  GemmArgs g{dy, W, dx, nullptr, M, N, K, lddy, ldw, lddx, beta, 1, nullptr};
  g.x3 = x3;
  gemm_launch<true, false>(s, g, x3 ? -1 : tile);   // tile = 2: 64 x 128 tiles (kbj_gemm.h: few 128 x 128 tiles quantise badly)
}
// dW[Nout][Nin] += dy^T x  (dy [R][Nout], x [R][Nin]); split-K over the R samples with atomics (dW pre-zeroed by the caller)
void linear_bwd_weight(kbj_ctx* ctx, hipStream_t s, bool x3, const float* dy, int lddy, const float* x, int ldx, float* dW, int lddw, int Nout, int Nin, int R) {
  // the long contraction (R = T*B samples) is split over the grid: 128x128 tiles when the output allows it, ~768 workgroups
  bool big = Nout >= 128 && Nin >= 128;
  int ts = big ? 128 : 64;
  int tiles = ((Nout + ts - 1) / ts) * ((Nin + ts - 1) / ts);
  int sk = std::max(2, std::min(256, g_splitk_wgs / std::max(1, tiles)));
  sk = std::max(2, std::min(sk, (R + 255) / 256));
  GemmArgs g{dy, x, dW, nullptr, Nout, Nin, R, lddy, ldx, lddw, 1, sk, nullptr};  // always the split-K path: accumulates into dW
  g.skws = sk_workspace(ctx, s, (size_t)sk * Nout * Nin);
  g.x3 = x3;
  gemm_launch<false, false>(s, g, big ? 1 : 0);
}

// two weight gradients that share dy in one launch: dW1 += dy^T x1, dW2 += dy^T x2 (x1, x2 [R][Nin] with the same ld)
void linear_bwd_weight2(kbj_ctx* ctx, hipStream_t s, bool x3, const float* dy, int lddy, const float* x1, const float* x2, int ldx, float* dW1, float* dW2, int lddw, int Nout, int Nin, int R) {
  bool big = Nout >= 128 && Nin >= 128;
  int ts = big ? 128 : 64;
  if (Nin % ts != 0) {  // the column split must fall on a tile boundary
    linear_bwd_weight(ctx, s, x3, dy, lddy, x1, ldx, dW1, lddw, Nout, Nin, R);
    linear_bwd_weight(ctx, s, x3, dy, lddy, x2, ldx, dW2, lddw, Nout, Nin, R);
    return;
  }
  int tiles = ((Nout + ts - 1) / ts) * (2 * Nin / ts);
  int sk = std::max(2, std::min(256, g_splitk_wgs / std::max(1, tiles)));
  sk = std::max(2, std::min(sk, (R + 255) / 256));
  GemmArgs g{dy, x1, dW1, nullptr, Nout, 2 * Nin, R, lddy, ldx, lddw, 1, sk, nullptr};
  g.B2 = x2; g.C2 = dW2; g.n1 = Nin;
  g.skws = sk_workspace(ctx, s, (size_t)sk * Nout * 2 * Nin);
  g.x3 = x3;
  gemm_launch<false, false>(s, g, big ? 1 : 0);
}
// column sums of X [M][N] (ld) added to out[N]: atomics over 512 row slices, or (deterministic) per-slice partials + ordered reduce
void colsum_acc(kbj_ctx* ctx, hipStream_t s, const float* X, int M, int N, int ld, float* out) {
  float* part = det_partials(ctx, s);
  colsum_launch(s, X, M, N, ld, out, part);
  if (part) reduce_rows_launch(s, part, DETP_ROWS, N, out);
}

// SEQ_UW, SEQ_FUSED_MAX_H, SEQ_MAX_H, dispatch_hidden and the grids of the recurrence / step launches: kbj_lstm_seq.h, kbj_lstm_bwd16.h (launch path)
constexpr int SEQ_COUNTER_WORDS = 256;   // hand-off words per recurrence launch (one per workgroup): the grid of a launch may not exceed it
constexpr int SEQ_COUNTER_TOTAL = 2 * MAXD * 4 * SEQ_COUNTER_WORDS;   // all launches of one call (forward + backward, MAXD layers, 4 nets): ONE clear

int seq_fwd(kbj_ctx* ctx, hipStream_t st, int H, const SeqFwdArgs& a0) {   // a0.counters: zeroed by the caller
  SeqFwdArgs a = a0;
  a.timeout_ticks = ws_of(ctx)->seq_timeout_ticks;
  KbjKernelTimer timer(st, a.X ? (a.ldx == KBJ_LD_ACTOR ? KBJ_KIND_SEQ_FWD_OBS : KBJ_KIND_SEQ_FWD_FUSED) : KBJ_KIND_SEQ_FWD, 2.0 * a.T * a.B * 4.0 * H * (H + (a.X ? (a.kx ? a.kx : H) : 0)));
  int drop = 0;
  if (ctx->set.seq_drop > 0 && seq_grid(H, a.B) > 1) { --ctx->set.seq_drop; drop = 1; }   // fault injection (KbjSettings::seq_drop)
  return seq_fwd_launch(st, H, a, drop) ? 0 : kbj_fail(ctx, "seq_fwd: the persistent LSTM kernels are built for hidden sizes 64, 128, ..., 512");
}
// row groups of a backward-recurrence launch (deterministic mode: rows of its per-row-group bias partials)
int seq_bwd_row_groups(int B, bool tiles16) { return tiles16 ? (B + BWD16_ROWS - 1) / BWD16_ROWS : (B + SEQ_ROWS - 1) / SEQ_ROWS; }
int seq_bwd(kbj_ctx* ctx, hipStream_t st, int H, const SeqBwdArgs& a0, bool tiles16 = false) {   // a0.counters: zeroed by the caller
  SeqBwdArgs a = a0;
  a.timeout_ticks = ws_of(ctx)->seq_timeout_ticks;
  KbjKernelTimer timer(st, tiles16 ? KBJ_KIND_SEQ_BWD16 : KBJ_KIND_SEQ_BWD, 2.0 * a.T * a.B * 4.0 * H * H);
  bool built;
  if (tiles16) {
    int drop = 0;
    if (ctx->set.seq_drop_bwd > 0 && seq_bwd16_grid(H, a.B) > 1 && H > BWD16_UNITS && H <= SEQ_FUSED_MAX_H) { --ctx->set.seq_drop_bwd; drop = 1; }   // fault injection (a launch without partners has nobody to time out)
    built = seq_bwd16_launch(st, H, a, drop);
  } else built = seq_bwd_launch(st, H, a);
  return built ? 0 : kbj_fail(ctx, "seq_bwd: the persistent LSTM kernels are built for hidden sizes 64, 128, ..., 512 (lstm_seq_bwd16_kernel: up to 256)");
}

// resident workgroups per CU of the recurrence kernel that fits worst, over EVERY recurrence kernel the schedule may launch for this
// hidden size (seq_blocks_per_cu, kbj_lstm_bwd16.h: all five kinds up to SEQ_FUSED_MAX_H, plain forward and wide backward above): in the
// gfx950 code object the fused forward is the largest (252 VGPRs / 86 KB of LDS at H = 256 against 176 / 52 KB for the backward)
hipError_t seq_min_blocks_per_cu(int H, int* out) {
  hipError_t e = seq_blocks_per_cu(SEQ_KIND_FWD_PLAIN, H, out);
  for (int k = 0, n = 0; k < SEQ_KIND_COUNT && e == hipSuccess; ++k)
    if (H <= SEQ_FUSED_MAX_H || k == SEQ_KIND_BWD32) { e = seq_blocks_per_cu((SeqKernelKind)k, H, &n); *out = std::min(*out, n); }
  return e;
}

// one LSTM layer step over many rows (kbj_lstm_seq.h lstm_step_kernel): grid = unit groups x row chunks, about one workgroup per CU
int lstm_step(kbj_ctx* ctx, hipStream_t st, int H, const StepArgs& a) {
  KbjKernelTimer timer(st, lstm_step_obs(a) ? KBJ_KIND_LSTM_STEP_OBS : KBJ_KIND_LSTM_STEP, 2.0 * a.M * 4.0 * H * (H + (a.kx ? a.kx : H)));
  return lstm_step_launch(st, H, a) ? 0 : kbj_fail(ctx, "lstm_step: the LSTM step kernels are built for hidden_size 64, 128, 192, 256");
}

}  // namespace

int kbj_nn_check_errors(kbj_ctx* ctx) {
  NnWs* w = ws_of(ctx);
  if (!w) return 0;
  if (w->seq_stamps) {  // diagnostics: average shader-clock cycles per phase of the actor layer-0 forward recurrence
    std::vector<long long> st((size_t)w->T * 6);
    if (hipMemcpy(st.data(), w->seq_stamps, st.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess && w->T > 2) {
      double d[6] = {0, 0, 0, 0, 0, 0};
      for (int t = 1; t < w->T - 1; ++t) { for (int k = 0; k < 5; ++k) d[k] += (double)(st[t * 6 + k + 1] - st[t * 6 + k]); d[5] += (double)(st[(t + 1) * 6] - st[t * 6 + 5]); }
      fprintf(stderr, "[kbj seq_fwd stamps, cycles/step] prefetch+wait %.0f stage %.0f mfma %.0f cell %.0f publish %.0f bulk-store %.0f\n",
              d[0] / (w->T - 2), d[1] / (w->T - 2), d[2] / (w->T - 2), d[3] / (w->T - 2), d[4] / (w->T - 2), d[5] / (w->T - 2));
    }
  }
  if (w->seq_bstamps) {
    std::vector<long long> st((size_t)w->T * 10 + 768);
    if (hipMemcpy(st.data(), w->seq_bstamps, st.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess && w->T > 3) {
      double d[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      int cnt = 0;
      for (int t = w->T - 3; t >= 1; --t, ++cnt) { for (int k = 0; k < 8; ++k) d[k] += (double)(st[t * 10 + k + 1] - st[t * 10 + k]); d[8] += (double)(st[(t - 1) * 10] - st[t * 10 + 8]); }
      fprintf(stderr, "[kbj seq_bwd stamps, cycles/step] wait %.0f chunk0-staged %.0f chunk1 %.0f chunk2 %.0f chunk3 %.0f last-mfma+reduce %.0f cell %.0f publish %.0f loop %.0f\n",
              d[0] / cnt, d[1] / cnt, d[2] / cnt, d[3] / cnt, d[4] / cnt, d[5] / cnt, d[6] / cnt, d[7] / cnt, d[8] / cnt);
      double ticks = (double)(st[1 * 10] - st[(w->T - 3) * 10]), wall = (double)(st[1 * 10 + 9] - st[(w->T - 3) * 10 + 9]);
      int wall_khz = 0;
      hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, ctx->device);
      if (wall_khz > 0) {   // per-workgroup entry / loop start / exit on the constant-rate clock
        const long long* g = st.data() + (size_t)w->T * 10;
        int nwg = ((w->B + SEQ_ROWS - 1) / SEQ_ROWS) * (w->H / (SEQ_UNITS * SEQ_UW));
        if (nwg > 256) nwg = 256;
        long long e0 = g[0], e1 = g[0], l1 = g[1], x0 = g[2], x1 = g[2];
        for (int i = 1; i < nwg; ++i) { e0 = std::min(e0, g[3 * i]); e1 = std::max(e1, g[3 * i]); l1 = std::max(l1, g[3 * i + 1]); x0 = std::min(x0, g[3 * i + 2]); x1 = std::max(x1, g[3 * i + 2]); }
        const double us = 1e3 / wall_khz;
        fprintf(stderr, "[kbj seq_bwd stamps] %d workgroups: last entry +%.1f us, last loop start +%.1f us, first exit +%.1f us, last exit +%.1f us (from the first entry)\n", nwg,
                (e1 - e0) * us, (l1 - e0) * us, (x0 - e0) * us, (x1 - e0) * us);
      }
      if (wall > 0 && wall_khz > 0) fprintf(stderr, "[kbj seq_bwd stamps] %.2f us/step, stamp counter at %.0f MHz\n", wall / wall_khz * 1e3 / cnt, ticks / wall * wall_khz * 1e-3);
    }
  }
  unsigned e[2] = {0, 0};
  if (hipMemcpy(e, w->seq_err, sizeof(e), hipMemcpyDeviceToHost) != hipSuccess) return kbj_fail(ctx, "hipMemcpy seq_err");
  if (e[0] || e[1]) {   // sticky until acknowledged here: clear, so the context stays usable (and destroyable) after the report
    hipMemset(w->seq_err, 0, sizeof(e));
    if (e[0]) return kbj_fail(ctx, "persistent LSTM kernel: inter-workgroup wait timed out (grid not fully resident?); the optimizer steps fed by it were skipped");
    return kbj_fail(ctx, "non-finite gradient norm: the optimizer step was skipped (parameters and moments unchanged)");
  }
  return 0;
}

// A pending kbj_ppo_prefetch is tied to the CONTENTS of the trajectory and of the index array it was given: every entry point that writes
// trajectory arrays (rollout, policy / env steps, GAE, rewards) calls this first - the stale gathers are ordered in front of the writer (they
// only read the trajectory, but their workspace rows must not be consumed) and the marker is cleared, so the next kbj_ppo_grad gathers afresh.
void kbj_nn_drop_prefetch(kbj_ctx* ctx) {
  NnWs* w = ws_of(ctx);
  if (!w || !w->prefetched_idx) return;
  hipStreamWaitEvent(ctx->stream, ctx->ev_prefetch, 0);
  w->prefetched_idx = nullptr; w->prefetched_traj = nullptr;
}

// THE place where the environment is read (besides kbj_rollout's per-call KBJ_ROLLOUT_PIPELINE): once per context, at the top of kbj_create
KbjSettings kbj_read_settings(const kbj_config& c) {
  auto flag = [](const char* name, bool dflt) { const char* v = getenv(name); return v ? atoi(v) != 0 : dflt; };
  auto number = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
  KbjSettings set;
  Sched& sc = set.sched;
  const bool wide = c.hidden_size > SEQ_FUSED_MAX_H;   // (SEQ_FUSED_MAX_H is a multiple of 64: the same answer for the padded size)
  sc.fold_actor = flag("KBJ_FOLD_ACTOR", true); sc.fold_critic = flag("KBJ_FOLD_CRITIC", true);
  sc.fuse_ih = flag("KBJ_SEQ_FUSE", true); sc.fuse_obs = sc.fuse_ih && flag("KBJ_SEQ_FUSE_OBS", true);
  sc.fused_critic_head = flag("KBJ_FUSED_CRITIC_HEAD", true); sc.rollout_step = flag("KBJ_ROLLOUT_STEP", true);
  sc.one_stream = flag("KBJ_ONE_STREAM", false); sc.debug_sync = flag("KBJ_DEBUG", false);
  sc.deterministic = c.deterministic != 0 || flag("KBJ_DETERMINISTIC", false);
  { const char* cl = getenv("KBJ_CRITIC_LANE"); sc.critic_on_caller = !(cl && std::string(cl) == "2nd"); }
  sc.bwd16 = flag("KBJ_BWD16", true) && !wide;   // wide layers keep lstm_seq_bwd_wide_kernel
  sc.gemm_x3 = (c.gemm_bf16x3 != 0 || flag("KBJ_GEMM_X3", false)) && !sc.deterministic;   // (the deterministic split-K slabs stay on the exact kernel)
  if (wide) sc.fuse_ih = sc.fuse_obs = sc.rollout_step = false;   // wide layers (SEQ_FUSED_MAX_H above)
  set.seq_drop = number("KBJ_DEBUG_DROP_SEQ_WG", 0);
  set.seq_drop_bwd = number("KBJ_DEBUG_DROP_SEQ_BWD_WG", 0);
  set.seq_timeout_ms = (set.seq_drop > 0 || set.seq_drop_bwd > 0) ? 20 : (int)SEQ_TIMEOUT_MS;
  if (getenv("KBJ_SEQ_TIMEOUT_MS")) set.seq_timeout_ms = std::max(1, std::min(30000, number("KBJ_SEQ_TIMEOUT_MS", 0)));
  set.seq_stamps = getenv("KBJ_SEQ_STAMPS") != nullptr; set.stamp_sel = number("KBJ_SEQ_STAMPS", 1);
  set.seq_bstamps = getenv("KBJ_SEQ_BSTAMPS") != nullptr; set.bstamp_sel = number("KBJ_SEQ_BSTAMPS", 0);
  return set;
}

namespace {

// ---- kbj_nn_create, step by step (each: 0 or kbj_fail) ----
int nn_layouts(kbj_ctx* ctx, NnWs* w) {
  const kbj_config& c = ctx->cfg_h;
  w->Hu = c.hidden_size; w->H = (c.hidden_size + 63) / 64 * 64; w->N = c.num_envs; w->B = c.batch_size; w->T = c.rollout_len;
  if (w->B <= 0 || w->B > w->N) return kbj_fail(ctx, "kbj_create: batch_size must be in [1, num_envs]");
  static_cast<ParamLayout&>(*w) = layout_params(c, w->H);
  w->user = layout_params(c, w->Hu);
  w->mirror = c.actor_mirror_loss_scale != 0.0f || c.critic_mirror_loss_scale != 0.0f;
  w->nnets = w->mirror ? 4 : 2;
  return 0;
}

// free hidden_size: descriptors of every leaf's place in the two layouts, internal copies of parameters, gradient and carries
int nn_padding(kbj_ctx* ctx, NnWs* w) {
  if (!w->padded()) return 0;
  std::vector<PadDesc> pd;
  const int Hu = w->Hu, Hi = w->H;
  for (int n = 0; n < 2; ++n) {
    const NetOff &a = w->user.net[n], &b = w->net[n];
    pd.push_back(PadDesc{a.w_in, b.w_in, 1, Hu, Hi, a.nin, a.nin});
    pd.push_back(PadDesc{a.b_in, b.b_in, 1, Hu, Hi, 1, 1});
    for (int l = 0; l < w->D; ++l) {
      pd.push_back(PadDesc{a.w_ih[l], b.w_ih[l], 4, Hu, Hi, Hu, Hi});
      pd.push_back(PadDesc{a.w_hh[l], b.w_hh[l], 4, Hu, Hi, Hu, Hi});
      pd.push_back(PadDesc{a.b[l], b.b[l], 4, Hu, Hi, 1, 1});
    }
    pd.push_back(PadDesc{a.w_out, b.w_out, 1, a.nout, a.nout, Hu, Hi});
    pd.push_back(PadDesc{a.b_out, b.b_out, 1, a.nout, a.nout, 1, 1});
  }
  w->npad = (int)pd.size();
  if (dalloc(ctx, *w, &w->pad_desc, pd.size())) return -1;
  if (hipMemcpy(w->pad_desc, pd.data(), pd.size() * sizeof(PadDesc), hipMemcpyHostToDevice) != hipSuccess) return kbj_fail(ctx, "hipMemcpy pad descriptors");
  if (dalloc(ctx, *w, &w->pparams, w->nparams) || dalloc(ctx, *w, &w->pgrad, w->nparams)) return -1;
  for (int k = 0; k < w->nnets; ++k)
    if (dalloc(ctx, *w, &w->phc[k], (size_t)2 * w->D * w->N * w->H) || dalloc(ctx, *w, &w->pc0[k], (size_t)2 * w->D * w->N * w->H)) return -1;
  return 0;
}

int nn_rollout_scratch(kbj_ctx* ctx, NnWs* w) {
  const size_t N = w->N, H = w->H;
  for (int n = 0; n < w->nnets; ++n) {
    if (dalloc(ctx, *w, &w->rX[n], N * H)) return -1;
    if (dalloc(ctx, *w, &w->rG[n], N * 4 * H)) return -1;
    if (dalloc(ctx, *w, &w->rOut[n], N * 40)) return -1;
    for (int l = 0; l < w->D; ++l) if (dalloc(ctx, *w, &w->rH[n][l], N * H)) return -1;
  }
  if (ctx->cfg_h.gae_tail_value && dalloc(ctx, *w, &w->tail_hc, 2 * (size_t)w->D * N * H)) return -1;
  if (ctx->cfg_h.gae_terminal_value && dalloc(ctx, *w, &w->term_rows, N * (size_t)w->net[1].ld_obs)) return -1;
  if (dalloc(ctx, *w, &w->joint_bias_d, KBJ_NU)) return -1;
  if (hipMemcpy(w->joint_bias_d, ctx->model_h.joint_bias, KBJ_NU * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return kbj_fail(ctx, "hipMemcpy joint_bias");
  return 0;
}

// the mirror branches' tables and buffers (rollout rows and minibatch), then everything a minibatch pass works in
int nn_training_buffers(kbj_ctx* ctx, NnWs* w) {
  const size_t N = w->N, H = w->H, B = w->B, T = w->T, R = T * B;
  if (w->mirror) {
    std::vector<MirrorEntry> ta, tc;
    build_mirror_tables(ctx->model_h, ta, tc, ctx->cfg_h.extra_obs_actor, ctx->cfg_h.extra_obs_critic);
    if (dalloc(ctx, *w, &w->mtab[0], ta.size()) || dalloc(ctx, *w, &w->mtab[1], tc.size())) return -1;
    if (hipMemcpy(w->mtab[0], ta.data(), ta.size() * sizeof(MirrorEntry), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(w->mtab[1], tc.data(), tc.size() * sizeof(MirrorEntry), hipMemcpyHostToDevice) != hipSuccess) return kbj_fail(ctx, "hipMemcpy mirror tables");
    if (dalloc(ctx, *w, &w->rObsM[0], N * w->net[0].ld_obs) || dalloc(ctx, *w, &w->rObsM[1], N * w->net[1].ld_obs)) return -1;
    float** rs[] = {&w->value_m, &w->dvalue_m, &w->zeroR};
    for (float** p : rs) if (dalloc(ctx, *w, p, R)) return -1;
    float** r20[] = {&w->y_m, &w->sd_m, &w->dy, &w->dy_m};
    for (float** p : r20) if (dalloc(ctx, *w, p, R * KBJ_NU)) return -1;
    if (dalloc(ctx, *w, &w->lpf0_m, B * KBJ_NU)) return -1;
    if (hipMemset(w->zeroR, 0, R * sizeof(float)) != hipSuccess) return kbj_fail(ctx, "hipMemset zeroR");
  }
  for (int n = 0; n < w->nnets; ++n) {
    TrainBufs& t = w->tb[n];
    if (dalloc(ctx, *w, &t.obs, R * w->net[n & 1].ld_obs)) return -1;
    if (dalloc(ctx, *w, &t.X0, R * H)) return -1;
    for (int l = 0; l < w->D; ++l) {
      if (dalloc(ctx, *w, &t.dGl[l], R * 4 * H)) return -1;
      if (dalloc(ctx, *w, &t.G[l], R * 4 * H)) return -1;
      if (dalloc(ctx, *w, &t.Hm[l], (T + 1) * B * H)) return -1;
      if (dalloc(ctx, *w, &t.Hout[l], R * H)) return -1;
      if (dalloc(ctx, *w, &t.Cm[l], (T + 1) * B * H)) return -1;
      if (dalloc(ctx, *w, &t.TanhC[l], R * H)) return -1;
    }
    if (dalloc(ctx, *w, &t.Out, R * 40)) return -1;
    if (dalloc(ctx, *w, &t.dOut, R * 40)) return -1;
    if (dalloc(ctx, *w, &t.dHa, R * H)) return -1;
    if (dalloc(ctx, *w, &t.dHb, R * H)) return -1;
  }
  float** small[] = {&w->keep, &w->logp_old, &w->val_old, &w->adv, &w->target, &w->logp, &w->ent, &w->value, &w->dlogp, &w->dvalue};
  for (float** p : small) if (dalloc(ctx, *w, p, R)) return -1;
  if (dalloc(ctx, *w, &w->act, R * KBJ_NU)) return -1;
  if (dalloc(ctx, *w, &w->y, R * KBJ_NU)) return -1;
  if (dalloc(ctx, *w, &w->sd, R * KBJ_NU)) return -1;
  if (dalloc(ctx, *w, &w->lpf0, B * KBJ_NU)) return -1;
  if (dalloc(ctx, *w, &w->stats, 16)) return -1;
  if (dalloc(ctx, *w, &w->Weff, (size_t)4 * H * w->net[0].ld_obs) || dalloc(ctx, *w, &w->beff, 4 * H)) return -1;
  for (int n = 0; n < w->nnets; ++n) if (dalloc(ctx, *w, &w->Zeff[n], 4 * H * w->net[n & 1].ld_obs)) return -1;
  for (int k = 0; k < 2; ++k) if (dalloc(ctx, *w, &w->WinP[k], H * w->net[k].ld_obs)) return -1;
  if (hipMemset(w->Weff, 0, (size_t)4 * H * w->net[0].ld_obs * sizeof(float)) != hipSuccess) return kbj_fail(ctx, "hipMemset Weff");
  if (dalloc(ctx, *w, &w->seq_counters, SEQ_COUNTER_TOTAL)) return -1;   // [phase: forward layer l = l, backward layer l = D + l][net][row group x unit group]
  if (dalloc(ctx, *w, &w->seq_err, 4)) return -1;
  if (ctx->set.seq_stamps && dalloc(ctx, *w, &w->seq_stamps, (size_t)T * 6)) return -1;
  if (ctx->set.seq_bstamps && dalloc(ctx, *w, &w->seq_bstamps, (size_t)T * 10 + 768)) return -1;
  if (hipMemset(w->seq_err, 0, 4 * sizeof(unsigned)) != hipSuccess) return kbj_fail(ctx, "hipMemset seq_err");
  return 0;
}

int nn_deterministic_workspaces(kbj_ctx* ctx, NnWs* w) {
  if (!w->sched.deterministic) return 0;
  for (int l = 0; l < 4; ++l) if (dalloc(ctx, *w, &w->detp[l], (size_t)DETP_ROWS * DETP_COLS)) return -1;
  return dalloc(ctx, *w, &w->detd, 2 * 512);
}

// Residency of the persistent recurrences: the workgroups of one launch spin on each other, and kbj_ppo_grad keeps TWO launches
// (actor-type and critic-type net, one per stream; the mirror branches queue behind them on the same two streams) in flight, so
// 2 x grid workgroups must be resident at once. Every other kernel of the schedule (GEMMs, heads) terminates on its own, so it can
// only delay a recurrence workgroup, never starve it. Slots = the occupancy query's answer for the WORST-fitting recurrence kernel
// of this hidden size. Independently, a launch owns SEQ_COUNTER_WORDS hand-off words (one per workgroup): a larger grid would write
// into the next launch's block, so it is refused whatever the occupancy says.
int nn_residency_check(kbj_ctx* ctx, NnWs* w) {
  const int H = w->H, B = w->B;
  const int grid = ((B + SEQ_ROWS - 1) / SEQ_ROWS) * (H / (SEQ_UNITS * SEQ_UW));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return kbj_fail(ctx, "hipGetDeviceProperties");
  const int cus = prop.multiProcessorCount;
  int per_cu = 0;
  if (!dispatch_hidden(H, [](auto) { return true; })) return kbj_fail(ctx, "kbj_create: hidden_size above 512 (persistent LSTM kernels)");
  if (seq_min_blocks_per_cu(H, &per_cu) != hipSuccess || per_cu < 1) return kbj_fail(ctx, "kbj_create: occupancy query of the persistent LSTM kernels failed");
  const long slots = (long)per_cu * cus;
  w->seq_grid = grid; w->seq_slots = (int)slots;
  char msg[320];
  if (grid > SEQ_COUNTER_WORDS) {
    snprintf(msg, sizeof(msg), "kbj_create: a persistent LSTM launch would need %d workgroups (batch_size / 32 x hidden_size / 32), the hand-off "
             "counters hold %d per launch: lower batch_size", grid, SEQ_COUNTER_WORDS);
    return kbj_fail(ctx, msg);
  }
  if (H > SEQ_FUSED_MAX_H && 2L * grid > slots) w->sched.one_stream = true;   // wide layers: one recurrence at a time
  if ((w->sched.one_stream ? 1L : 2L) * grid > slots) {
    snprintf(msg, sizeof(msg), "kbj_create: %s persistent LSTM launches need %ld resident workgroups, the device holds %ld "
             "(%d per CU x %d CUs): lower batch_size", w->sched.one_stream ? "the" : "two concurrent", (w->sched.one_stream ? 1L : 2L) * grid, slots, per_cu, cus);
    return kbj_fail(ctx, msg);
  }
  return 0;
}

}  // namespace

int kbj_nn_create(kbj_ctx* ctx) {
  NnWs* w = new NnWs(ctx->set.sched);
  ctx->nn_ws = w;
  if (nn_layouts(ctx, w) || nn_padding(ctx, w) || nn_rollout_scratch(ctx, w) || nn_training_buffers(ctx, w) || nn_deterministic_workspaces(ctx, w)) return -1;
  int wall_khz = 0;   // the settings' bound of the recurrences' waits in this device's wall_clock64 ticks
  if (hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || wall_khz <= 0) wall_khz = 100000;
  w->seq_timeout_ticks = (unsigned)std::min<long long>(0xFFFFFFFFll, (long long)ctx->set.seq_timeout_ms * wall_khz);
  return nn_residency_check(ctx, w);
}

void kbj_nn_destroy(kbj_ctx* ctx) {
  NnWs* w = ws_of(ctx);
  if (!w) return;
  for (void* p : w->allocs) hipFree(p);
  for (int l = 0; l < 4; ++l) if (w->skws[l]) hipFree(w->skws[l]);
  delete w;
  ctx->nn_ws = nullptr;
}

namespace {

// Lane hops. Every ordering between two lanes, of the rollout and of the update, is one of these: an event recorded on one stream, waited for
// on another - one packet each (a cross-queue wait costs the waiting queue ~7 us, 10-25 us when it has to stall: round 6), so a helper issues
// exactly the calls its name says and a call site that reuses a record (UpdatePlan::critic_fork_recorded; ev_obs, which implies ev_small) says so.
int ev_record(kbj_ctx* ctx, hipEvent_t ev, hipStream_t on) { KBJ_HIP(ctx, hipEventRecord(ev, on)); return 0; }
int ev_wait(kbj_ctx* ctx, hipStream_t st, hipEvent_t ev) { KBJ_HIP(ctx, hipStreamWaitEvent(st, ev, 0)); return 0; }
int hop(kbj_ctx* ctx, hipStream_t from, hipStream_t to, hipEvent_t ev) { return ev_record(ctx, ev, from) || ev_wait(ctx, to, ev) ? -1 : 0; }

// ---- free hidden_size: conversions at the ABI boundary of a padded context (NnWs::Hu != NnWs::H) ----
void pad_params(kbj_ctx* ctx, hipStream_t s, const float* user, float* internal) {
  NnWs& w = *ws_of(ctx);
  hipLaunchKernelGGL(pad_params_kernel, g1(w.nparams), dim3(256), 0, s, w.pad_desc, w.npad, const_cast<float*>(user), internal, w.nparams, 0);
}
void unpad_params(kbj_ctx* ctx, hipStream_t s, const float* internal, float* user) {
  NnWs& w = *ws_of(ctx);
  hipLaunchKernelGGL(pad_params_kernel, g1(w.nparams), dim3(256), 0, s, w.pad_desc, w.npad, user, const_cast<float*>(internal), w.nparams, 1);
}
// carries [D][2][N][width]: ws -> wd columns per row
void repitch_hc(kbj_ctx* ctx, hipStream_t s, const float* src, float* dst, int ws, int wd) {
  NnWs& w = *ws_of(ctx);
  const size_t rows = (size_t)2 * w.D * w.N;
  repitch_pad_launch(s, src, dst, rows, ws, wd);
}
// the caller's carry as an H-wide internal one (lpf state is not hidden-size dependent: shared)
kbj_carry pad_carry(kbj_ctx* ctx, hipStream_t s, const kbj_carry& c) {
  NnWs& w = *ws_of(ctx);
  kbj_carry p = c;
  for (int k = 0; k < 4; ++k)
    if (carry_hc(c, k) && w.phc[k]) { repitch_hc(ctx, s, carry_hc(c, k), w.phc[k], w.Hu, w.H); carry_hc(p, k) = w.phc[k]; }
  return p;
}
void unpad_carry(kbj_ctx* ctx, hipStream_t s, const kbj_carry& c) {
  NnWs& w = *ws_of(ctx);
  for (int k = 0; k < 4; ++k)
    if (carry_hc(c, k) && w.phc[k]) repitch_hc(ctx, s, w.phc[k], carry_hc(c, k), w.H, w.Hu);
}
// the trajectory with its start carries as H-wide internal copies
kbj_traj pad_traj_carry0(kbj_ctx* ctx, hipStream_t s, const kbj_traj& tr) {
  NnWs& w = *ws_of(ctx);
  kbj_traj p = tr;
  for (int k = 0; k < 4; ++k)
    if (traj_carry0(tr, k) && w.pc0[k]) { repitch_hc(ctx, s, traj_carry0(tr, k), w.pc0[k], w.Hu, w.H); traj_carry0(p, k) = w.pc0[k]; }
  return p;
}

// ---- the rollout (kbj_rollout, kbj_policy_step, kbj_critic_value, kbj_carry_reset): ONE plan per call, one function per phase ----
// A control step runs every net of the context once on one observation row: mirrored rows (mirror branches), input projection, the LSTM
// layers, the head. WHICH kernels a net runs, and on which lane, is decided once per entry-point call, in rollout_plan(); the phases of
// Rollout read the plan and never re-derive a decision.

// net n of the call (0 actor, 1 critic, 2 / 3 their mirror branches: the same weights on mirrored observation rows, with carries of their own)
//   lane          the stream the net's launches go to
//   type          n & 1: the parameter / offset set (NnWs::net), the mirror table
//   step_kernel   its layers run in lstm_step_kernel (fused [x | h] product + cell) on ping-pong h planes; false: one GEMM over [x | h] plus a
//                 cell kernel per layer, in place
//   folded0       layer-0 gates straight from the observation row through Weff / beff, no input projection (fold_actor_weights has prepared them)
//   tile          the tile selector its gate GEMMs pass to gemm_launch: -1 the launcher's choice, 0 = 64 x 64
//   head          what follows the top layer
//   mirrored      its observation rows are mirrored first (train.py:1463-1481, 1555-1560)
//   hc, lpf       its carries [D][2][N][H] and low-pass state [N][KBJ_NU] (null: the net has none) in the call's kbj_carry
//   X, G, Out, obs_m, rH   its scratch rows and its h planes' partners: private to the net, lanes never share them
//   terminal      between the env step and its carry reset the net values the terminal rows of the envs that timed out (the critic under
//                 kbj_config.gae_terminal_value; Rollout::terminal_value)
enum HeadKind {
  HEAD_SAMPLE,   // output projection + low-pass + sample + log-prob as one launch (the chain env -> actor -> env waits for it)
  HEAD_VALUE,    // output projection to the value, one launch
  HEAD_LPF,      // the mirrored actor only advances its low-pass state (no sample)
  HEAD_NONE      // the mirrored critic's value is only needed under the gradient; at rollout time only its carry advances
};
struct RolloutNet { hipStream_t lane; int type; bool step_kernel, folded0, mirrored, terminal; int tile; HeadKind head; float *hc, *lpf, *X, *G, *Out, *obs_m, **rH; };
// the call
//   serial   every net on the caller's stream: kbj_policy_step, kbj_critic_value, kbj_carry_reset; kbj_rollout under KBJ_ROLLOUT_PIPELINE=0
//   side     the lane of the critic and the mirror branches (serial: the caller's stream)
//   term_rows   kbj_config.gae_terminal_value: where the env phase writes the terminal critic rows [N][ld_critic] (its terminal form runs
//               instead of the plain one); null with the switch off - then nothing of the terminal value is launched anywhere
//   ev_term     the terminal rows are ONE scratch, rewritten by every env step on the caller's stream and read by the value kernel on the side
//               lane - the only buffer the two lanes share that is not indexed by the step. So the side lane records this event behind the
//               value kernel of step t and the caller's stream waits for it in front of env step t + 1 (Rollout::terminal_rows_free): however
//               far the side lane lags, no env step overwrites rows that are still to be read. Null where there is nothing to order: the
//               switch off, or a serial plan (one stream)
struct RolloutPlan { RolloutNet net[4]; int nnets; bool serial; hipStream_t side; float* term_rows; hipEvent_t ev_term; };

RolloutPlan rollout_plan(kbj_ctx* ctx, const kbj_carry& carry, bool serial) {
  NnWs& w = *ws_of(ctx); const Sched& sc = w.sched;
  RolloutPlan p{};
  p.nnets = w.nnets; p.serial = serial;
  // The actor -> env step -> carry reset chain runs on the caller's stream; the critic (and the mirror branches), which the env never waits
  // for, on a side lane: its small kernels and GEMMs slip into the env kernel's ramp-up / tail (-8.5 ms per iteration against the serial
  // order). (A two-lane software pipeline over env halves existed until round 4: with 12 env wavefronts per CU no GEMM workgroup can be
  // co-resident, the lanes only alternated - gone.)
  p.side = serial ? ctx->stream : ctx->side[0];
  p.term_rows = ctx->cfg_h.gae_terminal_value ? w.term_rows : nullptr;
  p.ev_term = p.term_rows && !serial ? ctx->ev_term : nullptr;
  const HeadKind heads[4] = {HEAD_SAMPLE, HEAD_VALUE, HEAD_LPF, HEAD_NONE};
  float* const lpf[4] = {carry.lpf_d, nullptr, carry.lpf_mirror_d, nullptr};
  for (int n = 0; n < p.nnets; ++n) {
    RolloutNet& q = p.net[n]; q.type = n & 1;
    q.lane = n == 0 ? ctx->stream : p.side;
    // Rollout-time layer steps run in lstm_step_kernel (fused [x | h] product + cell). Its output h cannot alias its input, so every h
    // plane of the carry has a ping-pong partner in the workspace: a step with parity 0 reads the caller's planes and writes the partners,
    // parity 1 the other way round. kbj_rollout alternates per control step; the caller's arrays hold the state again when it returns.
    // KBJ_ROLLOUT_STEP=0 (Sched::rollout_step): the previous form, one GEMM over [x | h] plus a cell kernel per layer, in place.
    // Only the actor proper (net 0) sits on the rollout's critical chain (env -> actor -> env). The critic and the mirror branches run on side
    // lanes under the env kernel, where the only free resources are those of its last, partial round of wavefronts (8192 envs = 2.67 rounds
    // of 12 per CU: 168 VGPRs per SIMD and ~58 KB of LDS per CU for the last third of the kernel): a 64x64-tile GEMM workgroup (4 waves x 84
    // VGPRs, 37 KB) fits there, a layer-step workgroup (8 waves x 220 VGPRs) does not and would run into the next actor chain instead. So the
    // side-lane nets keep the GEMM + cell form on small tiles (414 vs 418 ms per iteration).
    q.step_kernel = sc.rollout_step && n == 0;
    q.tile = sc.rollout_step && n > 0 ? 0 : -1;
    // The actor's input projection (65 -> H, no activation) feeds only layer 0's input product, so gates_0 = obs (W_ih0 W_in)^T +
    // (W_ih0 b_in + b_0), as in kbj_ppo_grad (inside the layer-step kernel only: the GEMM + cell form keeps the projection)
    q.folded0 = q.step_kernel && sc.fold_actor && w.net[0].ld_obs == KBJ_LD_ACTOR;
    q.head = heads[n]; q.mirrored = n >= 2;
    // The terminal value is the critic's (net 1), on its own lane: it needs the critic's carry as the step left it, so it sits in front of
    // that net's carry reset, behind the hop that brings the env step's done flags and terminal rows over.
    q.terminal = n == 1 && p.term_rows != nullptr;
    q.hc = carry_hc(carry, n); q.lpf = lpf[n];
    q.X = w.rX[n]; q.G = w.rG[n]; q.Out = w.rOut[n]; q.obs_m = q.mirrored ? w.rObsM[q.type] : nullptr; q.rH = w.rH[n];
  }
  return p;
}

// the rows of one control step: what the nets read and write at step t, what the env step writes for step t + 1
struct StepRows {
  const float *actor_obs, *critic_obs; float *aux, *action, *logp, *value, *actor_next, *critic_next, *aux_next, *qstate;
  uint32_t step_index; int argmax, parity;   // parity: which copy of the step-kernel nets' h planes is live (0: the caller's arrays)
  float* value_term;                         // row t of the terminal values [N] (RolloutPlan::term_rows), else null
};

// the sparse terminal-value launch (kbj_terminal_value.h) for N rows: `par` and `hc` [D][2][N][width] in the layout `o` at hidden size `width`
void terminal_value_launch(hipStream_t st, const float* par, const NetOff& o, int N, int width, int D, const float* hc, const float* rows, const float* done_d, int done_stride,
                           float* value) {
  TermValueArgs a{};
  a.params = par; a.rows = rows; a.hc = hc; a.done = done_d; a.done_stride = done_stride; a.value = value;
  a.N = N; a.H = width; a.D = D; a.nin = o.nin; a.ld = o.ld_obs;
  a.w_in = o.w_in; a.b_in = o.b_in; a.w_out = o.w_out; a.b_out = o.b_out;
  for (int l = 0; l < D; ++l) { a.w_ih[l] = o.w_ih[l]; a.w_hh[l] = o.w_hh[l]; a.b[l] = o.b[l]; }
  critic_terminal_value_launch(st, a);
}

// One call of the rollout half: the parameters (H wide), the plan, the seed - and the phases. Each returns 0 or what kbj_fail returned.
struct Rollout {
  kbj_ctx* ctx; const float* params; const RolloutPlan p; uint32_t seed;
  NnWs& w = *ws_of(ctx); const kbj_config& c = ctx->cfg_h; const int N = w.N, H = w.H;
  const HeadParams hp{c.min_std, c.max_std, c.var_scale, c.lpf_alpha, w.net[0].ld_obs};

  float* c_plane(const RolloutNet& q, int l) { return q.hc + (size_t)(2 * l + 1) * N * H; }
  float* h_plane(const RolloutNet& q, int l, bool partner) { return partner ? q.rH[l] : q.hc + (size_t)(2 * l) * N * H; }

  // phase: the folded actor weights w.Weff / w.beff for these parameters (RolloutNet::folded0)
  void fold_actor_weights(hipStream_t s) {
    if (!p.net[0].folded0) return;
    const NetOff& oa = w.net[0];
    GemmArgs g{params + oa.w_ih[0], params + oa.w_in, w.Weff, nullptr, 4 * H, oa.nin, H, H, oa.nin, oa.ld_obs, 0, 1, nullptr};
    gemm_launch<true, false>(s, g);
    matvec_launch(s, params + oa.w_ih[0], params + oa.b_in, params + oa.b[0], 4 * H, H, w.beff);
  }

  // phase: re-pitched input weights of the net types [k_lo, k_hi)
  // Rollout-time input projections read W_in [H][nin] with nin = 65 / 475 floats per row: no 16-byte alignment, which puts the GEMM on its element-wise
  // load path for that operand (the critic's 8192 x 256 x 475 product ran at 27 TFLOP/s, with four times the load instructions - beside an env kernel
  // that is bound by vector issue). As in the update (Update::input_projections): a re-pitched copy with the observation rows' stride, zeros behind column nin,
  // made once per rollout / policy step; the contraction then runs over the padded width (the rows' padding columns hold zeros: host/buffers.py).
  void repitch_input_weights(hipStream_t s, int k_lo = 0, int k_hi = 2) {
    for (int k = k_lo; k < k_hi; ++k) {
      const NetOff& o = w.net[k];
      if (o.nin != o.ld_obs) repitch_rows_launch(s, params + o.w_in, H, o.nin, o.ld_obs, w.WinP[k]);
    }
  }

  // phase: the net's observation rows, mirrored first for the mirror branches
  const float* observation_rows(const RolloutNet& q, const StepRows& v) {
    const float* obs = q.type == 0 ? v.actor_obs : v.critic_obs;
    if (!q.mirrored) return obs;
    mirror_rows_launch(q.lane, obs, q.obs_m, (size_t)N, w.net[q.type].ld_obs, w.mtab[q.type]);
    return q.obs_m;
  }

  // phase: input projection X = obs W_in^T + b_in through the aligned copy of W_in (repitch_input_weights), or the stored one where it is aligned
  void input_projection(const RolloutNet& q, const float* obs) {
    const NetOff& o = w.net[q.type];
    if (o.nin != o.ld_obs) linear_fwd(q.lane, obs, o.ld_obs, w.WinP[q.type], o.ld_obs, params + o.b_in, q.X, H, N, H, o.ld_obs, 0);
    else linear_fwd(q.lane, obs, o.ld_obs, params + o.w_in, o.nin, params + o.b_in, q.X, H, N, H, o.nin, 0);
  }

  // phase: the layers on lstm_step_kernel, from one copy of the h planes into the other; returns the top layer's output (null: failed)
  const float* layers_step_kernel(const RolloutNet& q, const float* obs, int parity) {
    const NetOff& o = w.net[q.type];
    const float* x = q.X;
    for (int l = 0; l < w.D; ++l) {
      float* h_out = h_plane(q, l, parity == 0);
      StepArgs sa{x, H, 0, params + o.w_ih[l], H, params + o.w_hh[l], params + o.b[l], h_plane(q, l, parity != 0), h_out, c_plane(q, l), N};
      if (l == 0 && q.folded0) { sa.X = obs; sa.ldx = o.ld_obs; sa.kx = o.nin; sa.Wih = w.Weff; sa.ldw = o.ld_obs; sa.bias = w.beff; }
      if (lstm_step(ctx, q.lane, H, sa)) return nullptr;
      x = h_out;
    }
    return x;
  }

  // phase: the layers as gate GEMM + cell kernel, in place in the carry; returns the top layer's output
  const float* layers_gemm_cell(const RolloutNet& q) {
    const NetOff& o = w.net[q.type];
    const float* x = q.X;
    for (int l = 0; l < w.D; ++l) {
      float *h = h_plane(q, l, false), *cc = c_plane(q, l);
      // gates = [x | h] [W_ih | W_hh]^T + b as ONE launch over the concatenated contraction (no read-modify-write of G)
      GemmArgs g{x, params + o.w_ih[l], q.G, params + o.b[l], N, 4 * H, 2 * H, H, H, 4 * H, 0, 1, nullptr};
      g.A2 = h; g.B2 = params + o.w_hh[l]; g.k1 = H;
      g.x3 = w.sched.gemm_x3 ? 1 : 0;
      gemm_launch<true, true>(q.lane, g, q.tile);
      CellFwdArgs2 ca;
      ca.a[0] = CellFwdArgs{q.G, cc, h, cc, nullptr, nullptr, nullptr, nullptr, N, H};
      lstm_cell_fwd_launch(q.lane, ca, 1);
      x = h;
    }
    return x;
  }

  // phase: the head on the top layer's output x (RolloutNet::head)
  void head(const RolloutNet& q, const float* x, const float* obs, const StepRows& v) {
    const NetOff& o = w.net[q.type];
    if (q.head == HEAD_SAMPLE)
      actor_head_fused_launch(q.lane, x, H, params + o.w_out, params + o.b_out, obs, q.lpf, w.joint_bias_d, hp, seed, (uint32_t)c.env_id_offset, v.step_index, v.argmax, N,
                              v.action, v.logp);
    else if (q.head == HEAD_VALUE) critic_value_fused_launch(q.lane, x, H, params + o.w_out, params + o.b_out, N, v.value);
    else if (q.head == HEAD_LPF) {
      linear_fwd(q.lane, x, H, params + o.w_out, H, params + o.b_out, q.Out, 40, N, o.nout, H, 0);
      actor_head_lpf_launch(q.lane, q.Out, obs, q.lpf, w.joint_bias_d, c.lpf_alpha, N, w.net[0].ld_obs);
    }
  }

  // one control step of net q on its lane: the phases above in order
  int net_step(const RolloutNet& q, const StepRows& v) {
    const float* obs = observation_rows(q, v);
    if (!q.folded0) input_projection(q, obs);
    const float* x = q.step_kernel ? layers_step_kernel(q, obs, v.parity) : layers_gemm_cell(q);
    if (!x) return -1;
    head(q, x, obs, v);
    return 0;
  }

  // carry <- 0 where done, on the net's lane; parity as StepRows: which copy of the h planes is live
  void carry_reset(const RolloutNet& q, const float* done_d, int done_stride, int parity) {
    CarryPlanes cp;
    cp.n = 2 * w.D;
    for (int l = 0; l < w.D; ++l) { cp.p[2 * l] = h_plane(q, l, q.step_kernel && parity != 0); cp.p[2 * l + 1] = c_plane(q, l); }
    carry_reset_launch(q.lane, cp, N, H, q.lpf, done_d, done_stride);
  }

  // phase: the values of the terminal rows the env step has just written, for the envs that timed out (0 elsewhere), from the net's carry
  // BEFORE its reset - one sparse launch (terminal_value_launch) on the net's lane, then the record that frees the scratch for the next env
  // step (RolloutPlan::ev_term). The critic never runs on the layer-step kernel (rollout_plan), so its live h planes are the carry's own.
  int terminal_value(const RolloutNet& q, const StepRows& v) {
    if (!q.terminal) return 0;
    terminal_value_launch(q.lane, params, w.net[q.type], N, H, w.D, q.hc, p.term_rows, v.aux + KBJ_AUX_DONE, KBJ_AUX_SIZE, v.value_term);
    return p.ev_term ? ev_record(ctx, p.ev_term, q.lane) : 0;
  }
  // phase: in front of an env step that is not the call's first - the caller's stream waits until the previous step's terminal rows have been read
  int terminal_rows_free(hipStream_t s, bool first_step) { return p.ev_term && !first_step ? ev_wait(ctx, s, p.ev_term) : 0; }

  // the h planes of the step-kernel nets back from their ping-pong partners into the caller's arrays, on the caller's stream
  int planes_home() {
    for (int n = 0; n < p.nnets; ++n)
      for (int l = 0; l < w.D && p.net[n].step_kernel; ++l)
        KBJ_HIP(ctx, hipMemcpyAsync(h_plane(p.net[n], l, false), h_plane(p.net[n], l, true), (size_t)N * H * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
  }

  // The critic's value of ONE observation row [N][ld_critic] from a COPY of its carries (kbj_critic_value; the tail pass of kbj_rollout for
  // kbj_config.gae_tail_value): critic_hc_d [D][2][N][hc_width] goes into w.tail_hc (re-pitched when the caller's hidden_size is not the kernels'),
  // then the critic's phases step the copy on the critic's lane: net_step of the plan's net 1 with another carry base, so the value is
  // bit-identical to the one a policy step writes from the same carries and row. The critic never runs on the layer-step kernel
  // (rollout_plan), so no ping-pong partner plane is involved; its scratch rows belong to the rollout phases alone (the update and
  // kbj_ppo_prefetch work in w.tb[] and the gather buffers). The caller has run repitch_input_weights for these parameters on a stream
  // ordered in front of that lane. Nets 0, 2 and 3 do not run: no other carry, no low-pass state moves.
  int critic_tail(const float* critic_obs_d, const float* critic_hc_d, int hc_width, float* value_d) {
    RolloutNet q = p.net[1];   // (w.tail_hc: allocated at kbj_create exactly when gae_tail_value is set; both callers have checked)
    q.hc = w.tail_hc;
    if (hc_width == H) KBJ_HIP(ctx, hipMemcpyAsync(w.tail_hc, critic_hc_d, (size_t)2 * w.D * N * H * sizeof(float), hipMemcpyDeviceToDevice, q.lane));
    else repitch_hc(ctx, q.lane, critic_hc_d, w.tail_hc, hc_width, H);
    StepRows v{};
    v.critic_obs = critic_obs_d; v.value = value_d;
    return net_step(q, v);
  }
};

// ---- the H-wide bodies of the entry points below (arguments validated; a padded context passes its internal copies) ----
// all nets' phases on the caller's stream, then the planes brought home (the new h sits in the partners)
int policy_step_body(kbj_ctx* ctx, const float* params_d, const float* actor_obs_d, const float* critic_obs_d, kbj_carry* carry, uint32_t seed,
                     uint32_t step_index, int argmax, float* action_d, float* logp_d, float* value_d) {
  kbj_nn_drop_prefetch(ctx);   // action / logp / value may be trajectory rows
  KbjTimed timed(ctx, true);
  Rollout r{ctx, params_d, rollout_plan(ctx, *carry, true), seed};
  r.repitch_input_weights(ctx->stream);
  r.fold_actor_weights(ctx->stream);   // per call, so that step-wise calls stay bit-identical to the rollout
  const StepRows v{actor_obs_d, critic_obs_d, nullptr, action_d, logp_d, value_d, nullptr, nullptr, nullptr, nullptr, step_index, argmax, 0};
  for (int n = 0; n < r.p.nnets; ++n) if (r.net_step(r.p.net[n], v)) return -1;
  if (r.planes_home()) return -1;
  KBJ_CHECK_LAUNCH(ctx, "kbj_policy_step");
  return 0;
}

// snapshot, fork, per step: actor / others / env / resets (the critic's behind its terminal values) / hop, tail value, join, home copy, rewards
int rollout_body(kbj_ctx* ctx, const float* params_d, kbj_carry* carry, uint32_t seed, uint32_t first_step_index, kbj_traj* tr) {
  NnWs& w = *ws_of(ctx);
  const size_t N = w.N, T = tr->T, la = w.net[0].ld_obs, lc = w.net[1].ld_obs, lx = KBJ_AUX_SIZE;
  hipStream_t s = ctx->stream;
  kbj_nn_drop_prefetch(ctx);
  // observation row T of the previous rollout is row 0 of this one
  const struct { float* a; size_t ld; } rows[3] = {{tr->actor_obs_d, la}, {tr->critic_obs_d, lc}, {tr->aux_d, lx}};
  for (const auto& r : rows) KBJ_HIP(ctx, hipMemcpyAsync(r.a, r.a + T * N * r.ld, N * r.ld * sizeof(float), hipMemcpyDeviceToDevice, s));
  // the start-carry snapshot: per pair of nets (actor, critic; their mirror branches) the two carries, then the pair's low-pass state
  for (int n = 0; n < w.nnets; n += 2) {
    for (int k = n; k < n + 2; ++k)
      KBJ_HIP(ctx, hipMemcpyAsync(traj_carry0(*tr, k), carry_hc(*carry, k), 2 * w.D * N * w.H * sizeof(float), hipMemcpyDeviceToDevice, s));
    KBJ_HIP(ctx, hipMemcpyAsync(n ? tr->carry0_lpf_mirror_d : tr->carry0_lpf_d, n ? carry->lpf_mirror_d : carry->lpf_d, N * KBJ_NU * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  const char* pipe_env = getenv("KBJ_ROLLOUT_PIPELINE");   // =0 (read per call, diagnostics): strictly serial on the caller's stream
  Rollout r{ctx, params_d, rollout_plan(ctx, *carry, pipe_env && atoi(pipe_env) == 0), seed};
  const RolloutPlan& p = r.p;
  r.fold_actor_weights(s);      // once: the parameters are fixed for the whole rollout
  r.repitch_input_weights(s);   // (ahead of the fork: the side lane's critic reads the copy)
  if (!p.serial && hop(ctx, s, p.side, ctx->ev_fork)) return -1;
  for (size_t t = 0; t < T; ++t) {
    const StepRows v{tr->actor_obs_d + t * N * la, tr->critic_obs_d + t * N * lc, tr->aux_d + t * N * lx, tr->action_d + t * N * KBJ_NU, tr->logp_d + t * N, tr->value_d + t * N,
                     tr->actor_obs_d + (t + 1) * N * la, tr->critic_obs_d + (t + 1) * N * lc, tr->aux_d + (t + 1) * N * lx,
                     tr->qstate_d ? tr->qstate_d + t * N * KBJ_QSTATE_SIZE : nullptr, first_step_index + (uint32_t)t, ctx->rollout_argmax, (int)(t & 1),
                     p.term_rows ? w.value_term + t * N : nullptr};
    const float* done = v.aux + KBJ_AUX_DONE;
    for (int n = 0; n < p.nnets; ++n) if (r.net_step(p.net[n], v)) return -1;   // the actor on the caller's stream, the others on the side lane
    if (r.terminal_rows_free(s, t == 0)) return -1;
    const int rc = kbj_env_step_all(ctx, s, v.action, v.aux, v.actor_next, v.critic_next, v.aux_next, v.qstate, p.term_rows);
    if (rc) return rc;
    r.carry_reset(p.net[0], done, KBJ_AUX_SIZE, (v.parity + 1) & 1);   // the planes step t + 1 reads
    if (!p.serial && hop(ctx, s, p.side, ctx->ev_side[0])) return -1;   // the side lane needs this step's done flags and the next critic observation
    for (int n = 1; n < p.nnets; ++n) {
      if (r.terminal_value(p.net[n], v)) return -1;
      r.carry_reset(p.net[n], done, KBJ_AUX_SIZE, (v.parity + 1) & 1);
    }
  }
  // kbj_config.gae_tail_value: V(s_T) for kbj_gae - the critic once more, on observation row T with a copy of the carries the last reset left, on the
  // critic's lane in front of the join (under the tail of the last env step's successors: the actor's carry copy-back and kbj_rewards)
  if (ctx->cfg_h.gae_tail_value && tr->value_tail_d && r.critic_tail(tr->critic_obs_d + T * N * lc, carry->critic_hc_d, w.H, tr->value_tail_d)) return -1;
  KBJ_CHECK_LAUNCH(ctx, "kbj_rollout");
  if (!p.serial && hop(ctx, p.side, s, ctx->ev_side[0])) return -1;   // join the side lane back into the caller's stream
  if ((T & 1) && r.planes_home()) return -1;   // an odd number of steps leaves the live h planes in the partners
  return kbj_rewards(ctx, tr->aux_d, (int)T, tr->reward_d, tr->reward_comps_d);
}

}  // namespace

extern "C" {

int kbj_mirror_table(const void* model_blob, size_t model_bytes, int critic, int32_t* src_h, float* mul_h, float* add_h) {
  if (!model_blob || !src_h || !mul_h || !add_h || model_bytes != sizeof(kbj_model)) return kbj_fail(nullptr, "kbj_mirror_table: bad argument");
  std::vector<MirrorEntry> ta, tc;
  build_mirror_tables(*reinterpret_cast<const kbj_model*>(model_blob), ta, tc);
  const std::vector<MirrorEntry>& t = critic ? tc : ta;
  for (size_t k = 0; k < t.size(); ++k) { src_h[k] = t[k].src; mul_h[k] = t[k].mul; add_h[k] = t[k].add; }
  return (int)t.size();
}

size_t kbj_param_count(const kbj_config* cfg) { return layout_params(*cfg, cfg->hidden_size).nparams; }
size_t kbj_actor_param_count(const kbj_config* cfg) { return layout_params(*cfg, cfg->hidden_size).nactor; }

int kbj_init_params(kbj_ctx* ctx, uint32_t seed, float* params_d) {
  if (!ctx || !params_d) return kbj_fail(ctx, "kbj_init_params: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  const ParamLayout& u = w.user;         // the caller's layout: fan-ins and offsets follow its hidden_size, not the kernels' padded one
  int H = w.Hu;
  uint32_t leaf = 0;
  auto fill = [&](size_t off, size_t n, int fan_in) {
    init_uniform_launch(ctx->stream, params_d + off, n, 1.0f / std::sqrt((float)fan_in), seed, leaf++);
  };
  for (int n = 0; n < 2; ++n) {
    const NetOff& o = u.net[n];
    fill(o.w_in, (size_t)H * o.nin, o.nin); fill(o.b_in, H, o.nin);
    for (int l = 0; l < w.D; ++l) { fill(o.w_ih[l], (size_t)4 * H * H, H); fill(o.w_hh[l], (size_t)4 * H * H, H); fill(o.b[l], (size_t)4 * H, H); }
    fill(o.w_out, (size_t)o.nout * H, H); fill(o.b_out, o.nout, H);
  }
  KBJ_CHECK_LAUNCH(ctx, "init_uniform_kernel");
  return 0;
}

int kbj_policy_step(kbj_ctx* ctx, const float* params_d, const float* actor_obs_d, const float* critic_obs_d, kbj_carry* carry, uint32_t seed,
                    uint32_t step_index, int argmax, float* action_d, float* logp_d, float* value_d) {
  if (!ctx || !params_d || !actor_obs_d || !critic_obs_d || !carry || !action_d || !logp_d || !value_d) return kbj_fail(ctx, "kbj_policy_step: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  if (mirror_arrays_missing(w.mirror, carry, nullptr)) return kbj_fail(ctx, "kbj_policy_step: the mirror losses are enabled, the carry needs the mirror-branch arrays");
  if (!w.padded()) return policy_step_body(ctx, params_d, actor_obs_d, critic_obs_d, carry, seed, step_index, argmax, action_d, logp_d, value_d);
  pad_params(ctx, ctx->stream, params_d, w.pparams);
  kbj_carry pc = pad_carry(ctx, ctx->stream, *carry);
  const int rc = policy_step_body(ctx, w.pparams, actor_obs_d, critic_obs_d, &pc, seed, step_index, argmax, action_d, logp_d, value_d);
  unpad_carry(ctx, ctx->stream, *carry);
  return rc;
}

int kbj_carry_reset(kbj_ctx* ctx, kbj_carry* carry, const float* done_d, int done_stride) {
  if (!ctx || !carry || !done_d) return kbj_fail(ctx, "kbj_carry_reset: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  if (mirror_arrays_missing(w.mirror, carry, nullptr)) return kbj_fail(ctx, "kbj_carry_reset: the mirror losses are enabled, the carry needs the mirror-branch arrays");
  const kbj_carry pc = w.padded() ? pad_carry(ctx, ctx->stream, *carry) : *carry;
  Rollout r{ctx, nullptr, rollout_plan(ctx, pc, true), 0};   // (the body: H wide, the caller's planes live)
  for (int n = 0; n < r.p.nnets; ++n) r.carry_reset(r.p.net[n], done_d, done_stride, 0);
  if (w.padded()) unpad_carry(ctx, ctx->stream, *carry);
  KBJ_CHECK_LAUNCH(ctx, "carry_reset_kernel");
  return 0;
}

int kbj_critic_value(kbj_ctx* ctx, const float* params_d, const float* critic_obs_d, const kbj_carry* carry, float* value_d) {
  if (!ctx || !params_d || !critic_obs_d || !carry || !carry->critic_hc_d || !value_d) return kbj_fail(ctx, "kbj_critic_value: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  if (!w.tail_hc) return kbj_fail(ctx, "kbj_critic_value: the context was created with kbj_config.gae_tail_value = 0 (the carry copy it steps is allocated for 1 only)");
  kbj_nn_drop_prefetch(ctx);   // value_d may be a trajectory array
  const float* p = params_d;
  if (w.padded()) { pad_params(ctx, ctx->stream, params_d, w.pparams); p = w.pparams; }   // (of the carries only the critic's is read: critic_tail re-pitches it into its copy)
  Rollout r{ctx, p, rollout_plan(ctx, *carry, true), 0};
  r.repitch_input_weights(ctx->stream, 1, 2);
  if (r.critic_tail(critic_obs_d, carry->critic_hc_d, w.Hu, value_d)) return -1;
  KBJ_CHECK_LAUNCH(ctx, "kbj_critic_value");
  return 0;
}

int kbj_critic_terminal_value(kbj_ctx* ctx, const float* params_d, const float* critic_term_d, const kbj_carry* carry, const float* done_d, int done_stride,
                              float* value_term_d) {
  if (!ctx || !params_d || !critic_term_d || !carry || !carry->critic_hc_d || !done_d || !value_term_d) return kbj_fail(ctx, "kbj_critic_terminal_value: null argument");
  if (done_stride < 1) return kbj_fail(ctx, "kbj_critic_terminal_value: done_stride must be positive");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  // the caller's own layout throughout: parameters and carry at its hidden_size, nothing padded or copied (kbj_terminal_value.h)
  terminal_value_launch(ctx->stream, params_d, w.user.net[1], w.N, w.Hu, w.D, carry->critic_hc_d, critic_term_d, done_d, done_stride, value_term_d);
  KBJ_CHECK_LAUNCH(ctx, "critic_terminal_value_kernel");
  return 0;
}

int kbj_set_terminal_values(kbj_ctx* ctx, float* value_term_d) {
  if (!ctx || !ctx->nn_ws) return kbj_fail(ctx, "kbj_set_terminal_values: null ctx");
  ws_of(ctx)->value_term = value_term_d;
  return 0;
}

// ---- deployment (convert.py init_fn / step_fn): kbj_deploy.h ----
int kbj_deploy_carry_size(const kbj_config* cfg) {
  if (!cfg) return kbj_fail(nullptr, "kbj_deploy_carry_size: null argument");
  return cfg->depth * 2 * cfg->hidden_size + KBJ_NU;
}

int kbj_deploy_init(kbj_ctx* ctx, int N, float* carry_d) {
  if (!ctx || !carry_d) return kbj_fail(ctx, "kbj_deploy_init: null argument");
  if (N <= 0) return kbj_fail(ctx, "kbj_deploy_init: N must be positive");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  KBJ_HIP(ctx, hipMemsetAsync(carry_d, 0, (size_t)N * kbj_deploy_carry_size(&ctx->cfg_h) * sizeof(float), ctx->stream));
  return 0;
}

int kbj_deploy_step(kbj_ctx* ctx, const float* actor_params_d, const kbj_deploy_inputs* in, int N, const float* carry_in_d, float* carry_out_d, float* action_d) {
  if (!ctx || !actor_params_d || !in || !in->joint_angles_d || !in->joint_angular_velocities_d || !in->projected_gravity_d || !in->gyroscope_d || !in->command_d ||
      !carry_in_d || !carry_out_d || !action_d)
    return kbj_fail(ctx, "kbj_deploy_step: null argument");
  if (N <= 0) return kbj_fail(ctx, "kbj_deploy_step: N must be positive");
  if (ctx->cfg_h.extra_obs_actor > 0)
    return kbj_fail(ctx, "kbj_deploy_step: the context has extra_obs_actor > 0; the deployed contract (convert.py:85-105) has the reference's 65 inputs and no place for user columns");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  const NnWs& w = *ws_of(ctx);
  const NetOff& o = w.user.net[0];        // the caller's layout, at its own hidden_size
  DeployArgs a{};
  a.params = actor_params_d; a.in = *in; a.carry_in = carry_in_d; a.carry_out = carry_out_d; a.action = action_d;
  a.model = ctx->model_d; a.alpha = ctx->cfg_h.lpf_alpha; a.H = w.Hu; a.D = w.D;
  a.w_in = o.w_in; a.b_in = o.b_in; a.w_out = o.w_out; a.b_out = o.b_out;
  for (int l = 0; l < w.D; ++l) { a.w_ih[l] = o.w_ih[l]; a.w_hh[l] = o.w_hh[l]; a.b[l] = o.b[l]; }
  actor_deploy_step_launch(ctx->stream, a, N);
  KBJ_CHECK_LAUNCH(ctx, "actor_deploy_step_kernel");
  return 0;
}

int kbj_rollout(kbj_ctx* ctx, const float* params_d, kbj_carry* carry, uint32_t seed, uint32_t first_step_index, kbj_traj* tr) {
  if (!ctx || !params_d || !carry || !tr) return kbj_fail(ctx, "kbj_rollout: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  if (tr->N != w.N || tr->T <= 0) return kbj_fail(ctx, "kbj_rollout: trajectory shape does not match the context");
  if (mirror_arrays_missing(w.mirror, carry, tr)) return kbj_fail(ctx, "kbj_rollout: the mirror losses are enabled, carry and trajectory need the mirror-branch arrays");
  if (ctx->cfg_h.gae_terminal_value && !w.value_term)
    return kbj_fail(ctx, "kbj_rollout: kbj_config.gae_terminal_value = 1 needs the [T][N] buffer of kbj_set_terminal_values, none is set");
  if (ctx->cfg_h.gae_terminal_value && tr->qstate_d)
    return kbj_fail(ctx, "kbj_rollout: kbj_config.gae_terminal_value = 1 with kbj_traj.qstate_d: no env step kernel writes both the state record and the terminal rows - "
                         "drop the record (record_state) or the terminal value");
  if (!w.padded()) return rollout_body(ctx, params_d, carry, seed, first_step_index, tr);
  // the H-wide schedule on internal copies; the caller's start-carry snapshot is taken here, at its own width
  const size_t ub = (size_t)2 * w.D * w.N * w.Hu * sizeof(float);
  for (int k = 0; k < w.nnets; ++k) {
    if (!traj_carry0(*tr, k) || !carry_hc(*carry, k)) return kbj_fail(ctx, "kbj_rollout: carry / trajectory start-carry array is NULL");
    KBJ_HIP(ctx, hipMemcpyAsync(traj_carry0(*tr, k), carry_hc(*carry, k), ub, hipMemcpyDeviceToDevice, ctx->stream));
  }
  pad_params(ctx, ctx->stream, params_d, w.pparams);
  kbj_carry pc = pad_carry(ctx, ctx->stream, *carry);
  kbj_traj pt = *tr;
  for (int k = 0; k < 4; ++k) traj_carry0(pt, k) = w.pc0[k];
  const int rc = rollout_body(ctx, w.pparams, &pc, seed, first_step_index, &pt);
  unpad_carry(ctx, ctx->stream, *carry);
  return rc;
}

int kbj_gae(kbj_ctx* ctx, const kbj_traj* tr, float* adv_d, float* target_d) {
  if (!ctx || !tr || !adv_d || !target_d) return kbj_fail(ctx, "kbj_gae: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  const kbj_config& c = ctx->cfg_h;
  if (c.gae_tail_value && !tr->value_tail_d)
    return kbj_fail(ctx, "kbj_gae: kbj_config.gae_tail_value = 1 needs kbj_traj.value_tail_d (kbj_rollout / kbj_critic_value fill it), it is NULL");
  if (c.gae_terminal_value && !ws_of(ctx)->value_term)
    return kbj_fail(ctx, "kbj_gae: kbj_config.gae_terminal_value = 1 needs the [T][N] buffer of kbj_set_terminal_values (kbj_rollout / kbj_critic_terminal_value fill it), none is set");
  kbj_nn_drop_prefetch(ctx);
  if (c.gae_terminal_value) {   // a truncation bootstraps from the recorded value of the terminal observation (implies gae_bootstrap_truncation: kbj_check_config)
    hipLaunchKernelGGL(gae_terminal_kernel, g1(tr->N, 64), dim3(64), 0, ctx->stream, tr->value_d, tr->reward_d, tr->aux_d, c.gae_tail_value ? tr->value_tail_d : nullptr,
                       ws_of(ctx)->value_term, tr->T, tr->N, c.gamma, c.lam, adv_d, target_d);
    KBJ_CHECK_LAUNCH(ctx, "gae_terminal_kernel");
    return 0;
  }
  if (c.gae_bootstrap_truncation || c.gae_tail_value) {   // the selectable boundary conventions (kbj.h); the default below is untouched by them
    hipLaunchKernelGGL(gae_boundary_kernel, g1(tr->N, 64), dim3(64), 0, ctx->stream, tr->value_d, tr->reward_d, tr->aux_d, c.gae_tail_value ? tr->value_tail_d : nullptr,
                       tr->T, tr->N, c.gamma, c.lam, (int)c.gae_bootstrap_truncation, adv_d, target_d);
    KBJ_CHECK_LAUNCH(ctx, "gae_boundary_kernel");
    return 0;
  }
  hipLaunchKernelGGL(gae_kernel, g1(tr->N, 64), dim3(64), 0, ctx->stream, tr->value_d, tr->reward_d, tr->aux_d, tr->T, tr->N, c.gamma, c.lam, adv_d, target_d);
  KBJ_CHECK_LAUNCH(ctx, "gae_kernel");
  return 0;
}

}  // extern "C"

namespace {

// the parameter-independent gathers in front of the first recurrences: actor observation rows, keep flags, start carries (and low-pass state)
int head_gathers(kbj_ctx* ctx, hipStream_t st, const kbj_traj* tr, const int32_t* idx) {
  NnWs& w = *ws_of(ctx);
  const int T = tr->T, N = tr->N, H = w.H, B = w.B, R = T * B, D = w.D;
  const int lda = w.net[0].ld_obs;
  gather_rows_launch(st, tr->actor_obs_d, idx, T, N, B, lda, lda, w.tb[0].obs, lda);   // (w.tb[0].obs is an allocation of its own: 16-byte aligned)
  GatherSmallArgs gs{tr->action_d, nullptr, nullptr, nullptr, nullptr, tr->aux_d, w.act, w.logp_old, w.val_old, w.adv, w.target, w.keep};
  gather_small_launch(st, gs, idx, T, N, B, KBJ_NU + 4, KBJ_NU + 5);   // keep flags: all the recurrences need of these
  if (mirror_arrays_missing(w.mirror, nullptr, tr)) return kbj_fail(ctx, "PPO pass: the mirror losses are enabled, the trajectory needs the mirror-branch carries");
  GatherCarryArgs gc;
  gc.nplanes = 0;
  for (int n = 0; n < w.nnets; ++n)
    for (int l = 0; l < D; ++l) {  // carry at the start of the trajectory: [N][H] planes h, c of every layer
      gc.src[gc.nplanes] = traj_carry0(*tr, n) + (size_t)(2 * l) * N * H; gc.dst[gc.nplanes++] = w.tb[n].Hm[l];
      gc.src[gc.nplanes] = traj_carry0(*tr, n) + (size_t)(2 * l + 1) * N * H; gc.dst[gc.nplanes++] = w.tb[n].Cm[l];
    }
  gc.nlpf = 0;
  gc.src[gc.nplanes] = tr->carry0_lpf_d; gc.dst[gc.nplanes] = w.lpf0; gc.nlpf++;
  if (w.mirror) { gc.src[gc.nplanes + 1] = tr->carry0_lpf_mirror_d; gc.dst[gc.nplanes + 1] = w.lpf0_m; gc.nlpf++; }
  gather_carry_launch(st, gc, idx, B, H);
  return 0;
}

// ---- the PPO update (kbj_ppo_grad, kbj_ppo_forward, kbj_ppo_prefetch): ONE plan per call, named lane hops, one function per phase --------
// A minibatch pass gathers the minibatch (observations, actions, keep flags, start-of-trajectory carries; for the gradient also the old
// log-probs / values, advantages and targets), prepares the folded actor weights, runs the nets forward through time (afterwards
// w.tb[n].Hout[D-1] holds the top layer's outputs and the BPTT stash is in place), and - kbj_ppo_grad - the heads, losses and the way back.
// WHERE every launch goes is decided once, in update_plan(); the phases below read the plan and never re-derive a decision.

// net n of the call (0 actor, 1 critic, 2 / 3 their mirror branches: same weights, queued behind nets 0, 1 on the same lanes)
//   lane          the net's chain: actor-type nets on one lane, critic-type nets on the other; one of the two is the caller's stream, the other the context's second
//   side          the net's side lane: work that hangs off the chain (weight-gradient GEMMs, bias sums); on one stream it IS the lane
//   type          n & 1: the parameter / offset set (NnWs::net) and the per-type side lanes and events
//   folded0       layer 0 goes backwards through Z = dG0^T obs, without dX0 (Sched::fold_actor; critic-type nets: and Sched::fold_critic)
//   fwd_folded0   forwards as well: gates_0 = obs Weff^T + beff, no input projection (actor-type nets; the critic's fold is a backward formulation only)
//   tail_on_lane  the net's layer-0 weight-gradient work, and the pair of the layer above it, run on the net's OWN lane (update_plan says why)
struct NetPlan { hipStream_t lane, side; int type; bool folded0, fwd_folded0, tail_on_lane; };
// the call
//   two_lanes             !Sched::one_stream
//   gather_late           the critic's gathered observation copy is made on its side lane, under the recurrences
//   fused_critic_head     critic head, value loss and head backward as ONE kernel on the critic's lane
//   fuse_ih, fuse_obs     forward input products inside the persistent recurrences
//   critic_fork_recorded  the critic lane's record behind its loss doubles as the fork of its side lane
//   ev_critic_loss        what the metrics launch at the end of the actor's lane waits for
struct UpdatePlan {
  NetPlan net[4];
  int nnets;
  bool two_lanes, gather_late, fused_critic_head, fuse_ih, fuse_obs, critic_fork_recorded;
  hipEvent_t ev_critic_loss;
};

UpdatePlan update_plan(kbj_ctx* ctx) {
  const NnWs& w = *ws_of(ctx); const Sched& sc = w.sched;
  UpdatePlan p{};
  p.nnets = w.nnets; p.two_lanes = !sc.one_stream;
  // The large critic observation block (97 MB per minibatch, 45 us at HBM speed): the forward pass reads it once, through the critic's
  // input projection - which fetches its rows straight from the trajectory through the minibatch's indices (GemmArgs::a_idx) - so the
  // gathered copy, which the backward pass and the mirror branch want, is made on the critic's side lane, off the chain that starts the
  // critic's first recurrence. (One stream, mirror branches or an unfolded actor: gathered in front of the projection as before.)
  p.gather_late = p.two_lanes && !w.mirror && sc.fold_actor;
  // Without the mirror branches the critic's one-output head, the value half of the loss and the head's backward are ONE kernel on the
  // critic's lane (critic_head_kernel: ~30 us instead of two degenerate GEMMs and three small kernels, ~220 us, on the longer chain).
  p.fused_critic_head = sc.fused_critic_head && !w.mirror && w.net[1].nout == 1;
  // forward: the K = H input projections (x W_ih^T + b) run inside the persistent recurrence, their MFMAs placed around the flag poll and
  // the h-tile fetch where the matrix pipe idles (kbj_lstm_seq.h FUSE): a fused launch takes 1.11 instead of 0.88 ms, the 0.41-0.48 ms
  // GEMM in front of it and its 210 MB round trip of G disappear: ppo_grad 7.72 -> 7.47 ms. Sched::fuse_ih = false: separate GEMMs.
  p.fuse_ih = sc.fuse_ih;
  // the folded actor layer 0 the same way (observation row x Weff inside the recurrence, 17 k-steps): Sched::fuse_obs = false keeps the GEMM
  p.fuse_obs = sc.fuse_obs && w.net[0].ld_obs == KBJ_LD_ACTOR;
  // The metrics line is nobody's input. It used to be a one-thread launch on a side lane behind the losses - where every CU is about to be taken by the
  // backward recurrences (250 registers x 2 wavefronts per SIMD), so in most minibatches it sat dispatched-but-unplaced for ~450 us (2.9 % of the
  // summed kernel time in a rocprofv3 summary, and the side lane's next launch queued behind it): the same "waiting for a wave slot" artefact as the
  // pause kernel of rounds 4-5. It now runs at the END of the actor's lane (lane_tails), behind an event recorded on the critic's lane after its loss half.
  // The critic lane's record doubles as the fork of its side lane when nothing is launched on that lane in between - the fused head: one packet.
  // The event is then ev_side[1], which the join of the critic's side lane RE-RECORDS at the end of the call (projection_grads_and_joins): the
  // actor lane's wait in lane_tails is for the end of the critic's side lane - which it has just waited for when the critic's bias terms ran
  // on its own lane - not for the loss. Harmless (later in the same chain) and redundant there; the packet stays until a measured change
  // removes it. Without the fused head (or on one stream, where nothing waits) it is an event of its own: the wait is for the loss half,
  // which fired ~3 ms before.
  p.critic_fork_recorded = p.two_lanes && p.fused_critic_head;
  p.ev_critic_loss = p.critic_fork_recorded ? ctx->ev_side[1] : ctx->ev_critic_loss;
  const int caller_type = sc.critic_on_caller ? 1 : 0;   // the net type whose lane is the caller's stream (Sched::critic_on_caller, kbj_ctx.h)
  for (int n = 0; n < p.nnets; ++n) {
    NetPlan& q = p.net[n]; q.type = n & 1;
    q.lane = p.two_lanes && q.type != caller_type ? ctx->stream2 : ctx->stream;
    q.side = p.two_lanes ? ctx->side[q.type] : q.lane;
    q.folded0 = sc.fold_actor && (q.type == 0 || sc.fold_critic);
    q.fwd_folded0 = q.folded0 && q.type == 0;
    // The last thing a lane does - layer 0 of its net - needs no side lane: nothing is left on the net's lane for the weight
    // gradients to run beside, and a cross-lane hop costs 15-20 us each way (fork + join) in the minibatch's tail. (Not with mirror
    // branches: two nets per lane then read-modify-write the same dW_ih0 through their small products, which only the shared side
    // lane orders.)
    q.tail_on_lane = !w.mirror && q.folded0;
  }
  return p;
}

// the net's side lane starts behind what its lane has queued so far (one stream: stream order is the order); ev_record / ev_wait / hop: above the rollout
int fork_side(kbj_ctx* ctx, const UpdatePlan& p, const NetPlan& q) { return p.two_lanes ? hop(ctx, q.lane, q.side, ctx->ev_side[q.type]) : 0; }

// One call of the update: the caller's arguments (adv, target, grad: kbj_ppo_grad only; grad == nullptr is the forward-only pass), the
// minibatch's dimensions (R = T * B rows), the constants of the actor's head and of the loss, the plan - and the phases, in the order
// ppo_forward_body / ppo_grad_body call them. Each returns 0 or what kbj_fail returned.
struct Update {
  kbj_ctx* ctx; const float* params; const kbj_traj* tr; const int32_t* idx; const float *adv, *target; float* grad;   // what a body below passes in; the rest follows from it
  NnWs& w = *ws_of(ctx); const Sched& sc = w.sched; const kbj_config& c = ctx->cfg_h; const UpdatePlan p = update_plan(ctx);
  const int T = tr->T, N = tr->N, H = w.H, B = w.B, R = T * B, D = w.D;
  const HeadParams hp{c.min_std, c.max_std, c.var_scale, c.lpf_alpha, w.net[0].ld_obs};
  const PpoParams pp{c.clip_param, c.value_clip, c.value_loss_coef, c.entropy_coef, c.log_ratio_clip, c.adv_eps};
  bool bias_done[2] = {false, false};   // the layer-0 bias terms of net type k have run on the net's own lane (backward_layer); if not, lane_tails runs them

  // phase: lane setup and counter clear
  int lanes_begin() {
    // hand-off counters of all eight (sixteen with the mirror branches) recurrence launches of this call: one clear, ahead of both lanes
    // (kbj_ppo_grad leaves them cleared: each lane clears its nets' blocks behind its last recurrence, off the head of the next minibatch's chain)
    if (!w.counters_clean) KBJ_HIP(ctx, hipMemsetAsync(w.seq_counters, 0, SEQ_COUNTER_TOTAL * sizeof(unsigned), ctx->stream));
    w.counters_clean = false;
    return hop(ctx, ctx->stream, ctx->stream2, ctx->ev_fork);
  }

  // phase: folded-weight preparation
  // (first on the actor's lane, ahead of the gathers: the two small launches depend on the parameters only, and behind the gathers they
  // queue for CU slots behind the 800 workgroups of the critic's input projection - 87 us on the actor's chain instead of ~25)
  int folded_weights() {
    if (!p.net[0].fwd_folded0) return 0;
    // The actor's input projection (65 -> H, no activation) feeds only layer 0's input GEMM, so gates_0 = obs (W_ih0 W_in)^T +
    // (W_ih0 b_in + b_0): a 65-deep contraction instead of 65 -> H -> 4H (6.8 instead of 28.5 GFLOP per minibatch forward, and
    // 6.8 instead of 55 GFLOP backward). Same function, different rounding order (inside the parity tolerances).
    const NetOff& oa = w.net[0];
    GemmArgs g{params + oa.w_ih[0], params + oa.w_in, w.Weff, nullptr, 4 * H, oa.nin, H, H, oa.nin, oa.ld_obs, 0, 1, nullptr};
    gemm_launch<true, false>(p.net[0].lane, g);
    matvec_launch(p.net[0].lane, params + oa.w_ih[0], params + oa.b_in, params + oa.b[0], 4 * H, H, w.beff);
    return 0;
  }

  // the critic's observation rows of the minibatch, gathered (early on its lane, or late on its side lane: UpdatePlan::gather_late)
  void gather_critic_obs(hipStream_t st, int ld) { gather_rows_launch(st, tr->critic_obs_d, idx, T, N, B, ld, ld, w.tb[1].obs, ld); }

  // phase: gathers - the head gathers on the actor's lane (unless prefetched), the small ones and the clears on its side lane, the critic's
  // observations on its lane unless they are gathered late (input_projections), the mirrored observation rows
  int gathers() {
    const hipStream_t s = p.net[0].lane, sm = p.net[0].side;
    if (!p.gather_late) gather_critic_obs(p.net[1].lane, w.net[1].ld_obs);
    // What the FIRST recurrences read besides the parameters - the actor's observation rows, the keep flags, the start carries - depends on
    // the trajectory and the indices only. kbj_ppo_prefetch has queued these gathers behind the end of the previous kbj_ppo_grad, on a
    // side lane, where they run under the optimizer step and the folded-weight preparation instead of between them and the first recurrence.
    // A pending hint is ALWAYS waited for, matching or not: its gathers write the same workspace rows (observation copy, keep flags, start
    // carries) from a side lane, so a call with other arguments must order its own gathers behind them before it overwrites them.
    const bool pending = w.prefetched_idx != nullptr;
    const bool prefetched = pending && w.prefetched_idx == idx && w.prefetched_traj == tr && p.two_lanes;
    w.prefetched_idx = nullptr; w.prefetched_traj = nullptr;
    if ((pending && ev_wait(ctx, s, ctx->ev_prefetch)) || (!prefetched && head_gathers(ctx, s, tr, idx))) return -1;
    // Nothing on the forward path needs the rest: actions, old log-probs / values, advantages, targets, the advantage statistics and the
    // cleared accumulators (gradient, folded layer-0 products) are wanted at the loss, two recurrences later. They run on the actor's
    // side lane, idle until the backward pass, instead of in front of the first recurrence (where they were ~170 us of a 6 ms
    // minibatch with the matrix cores idle); both net lanes wait for them behind their last forward recurrence, and the side lanes
    // fork from the net lanes after that point, so every later reader and accumulator is ordered behind the clears.
    if (p.two_lanes && ev_wait(ctx, sm, ctx->ev_fork)) return -1;
    GatherSmallArgs gs{tr->action_d, grad ? tr->logp_d : nullptr, grad ? tr->value_d : nullptr, adv, target, tr->aux_d, w.act, w.logp_old, w.val_old, w.adv, w.target, w.keep};
    gather_small_launch(sm, gs, idx, T, N, B, 0, KBJ_NU + 4);
    if (grad) {
      KBJ_HIP(ctx, hipMemsetAsync(w.stats, 0, 16 * sizeof(double), sm));
#ifndef KBJ_NO_TAIL_CLEAN
      w.sumsq_clean = true;
#endif
      // (ordered in front of the end of this call on every lane: both net lanes wait for ev_small, the caller's stream joins them)
      if (w.ext_adv_sums) {   // global-batch statistics from the caller (all-reduced over the data-parallel ranks)
        KBJ_HIP(ctx, hipMemcpyAsync(w.stats, w.ext_adv_sums, 2 * sizeof(double), hipMemcpyDeviceToDevice, sm));
        KBJ_HIP(ctx, hipMemcpyAsync(w.stats + 11, w.ext_adv_sums + 2, sizeof(double), hipMemcpyDeviceToDevice, sm));
      } else {
        adv_stats_launch(sm, w.adv, R, w.stats, sc.deterministic ? w.detd : (double*)nullptr);
        if (sc.deterministic) reduce_double_launch(sm, w.detd, ADV_STATS_BLOCKS, 2, w.stats);
      }
      KBJ_HIP(ctx, hipMemsetAsync(grad, 0, w.nparams * sizeof(float), sm));
      for (int n = 0; n < p.nnets; ++n)
        if (p.net[n].folded0) KBJ_HIP(ctx, hipMemsetAsync(w.Zeff[n], 0, (size_t)4 * H * w.net[p.net[n].type].ld_obs * sizeof(float), sm));
    }
    // ev_join: the critic's lane needs keep / carries (gathered above on the actor's lane) before its first recurrence - not before its input
    // projection, which only reads its own gather: the wait sits behind the projections (input_projections)
    if ((p.two_lanes && ev_record(ctx, ctx->ev_small, sm)) || ev_record(ctx, ctx->ev_join, s)) return -1;
    if (w.mirror)   // mirrored observation rows: actor's on its lane, critic's behind its gather
      for (int k = 0; k < 2; ++k)
        mirror_rows_launch(p.net[k].lane, w.tb[k].obs, w.tb[2 + k].obs, (size_t)R, w.net[k].ld_obs, w.mtab[k]);
    return 0;
  }

  // phase: input projections X0 = obs W_in^T + b_in of the nets that have one forwards (launch order: net-major here, layer-major over the nets below)
  int input_projections() {
    for (int n = 0; n < p.nnets; ++n) {
      const NetPlan& q = p.net[n]; const NetOff& o = w.net[q.type];
      if (q.fwd_folded0) continue;   // layer-0 gates come straight from the observations
      // The stored rows of W_in are nin (65 / 475) floats long - no 16-byte alignment, which would put the GEMM on
      // its element-wise load path for this operand (55 instead of ~90 TF for the critic's 12 GFLOP, at the head of the longer chain): a
      // re-pitched copy with the observation rows' stride (zeros behind column nin, as in the observation rows) is made first; the
      // contraction then runs over the padded width
      if (n < 2) repitch_rows_launch(q.lane, params + o.w_in, H, o.nin, o.ld_obs, w.WinP[q.type]);
      if (n == 1 && p.gather_late) {
        GemmArgs g{tr->critic_obs_d, w.WinP[1], w.tb[1].X0, params + o.b_in, R, H, o.ld_obs, o.ld_obs, o.ld_obs, H, 0, 1, nullptr};
        g.a_idx = idx; g.a_B = B; g.a_N = N; g.x3 = sc.gemm_x3 ? 1 : 0;
        gemm_launch<true, true>(q.lane, g, sc.gemm_x3 ? -1 : 2);   // 64 x 128 tiles (kbj_gemm.h: 800 tiles of 128 x 128 are 1.56 rounds paid as 2)
        // the copy under the recurrences, on the critic's side lane. It starts behind the ACTOR lane's head (ev_join: the folded-weight preparation
        // and, without a prefetch hint, the head gathers - about when the projection ends; beside it the two would share HBM: 175 instead of 144 us
        // for the GEMM) and behind the side-lane gathers (ev_small), so that ev_obs implies both and the critic's lane - the chain a minibatch
        // waits for - carries ONE event wait in front of its loss instead of a record and two waits (each costs the queue ~7 us, round 6)
        if (ev_wait(ctx, q.side, ctx->ev_join) || ev_wait(ctx, q.side, ctx->ev_small)) return -1;
        if (grad) gather_critic_obs(q.side, o.ld_obs);   // the forward-only pass never reads the copy
        if (ev_record(ctx, ctx->ev_obs, q.side)) return -1;
        continue;
      }
      linear_fwd(q.lane, w.tb[n].obs, o.ld_obs, w.WinP[q.type], o.ld_obs, params + o.b_in, w.tb[n].X0, H, R, H, o.ld_obs, 0);
    }
    if (p.two_lanes && ev_wait(ctx, p.net[1].lane, ctx->ev_join)) return -1;   // keep / carries gathered on the actor's lane
    return 0;
  }

  // phase: forward through time, each net on its lane (the recurrences are latency bound, so the two lanes overlap); layer-major over the nets.
  // On return the two lanes are still forked (lane_tails / ppo_forward_body join them).
  int forward_recurrences() {
    const int stamp_sel = ctx->set.stamp_sel;   // diagnostics build: 1 + net + 2 * layer picks the stamped forward launch
    const int stamp_net = (stamp_sel - 1) & 1, stamp_layer = ((stamp_sel - 1) >> 1) & 1;
    for (int l = 0; l < D; ++l) {
      for (int n = 0; n < p.nnets; ++n) {
        const NetPlan& q = p.net[n]; const NetOff& o = w.net[q.type]; TrainBufs& t = w.tb[n];
        if (q.fwd_folded0 && l == 0) { if (!p.fuse_obs) linear_fwd(q.lane, t.obs, o.ld_obs, w.Weff, o.ld_obs, w.beff, t.G[0], 4 * H, R, 4 * H, o.nin, 0); }
        else if (!p.fuse_ih) linear_fwd(q.lane, l == 0 ? t.X0 : t.Hout[l - 1], H, params + o.w_ih[l], H, params + o.b[l], t.G[l], 4 * H, R, 4 * H, H, 0);
      }
      for (int n = 0; n < p.nnets; ++n) {
        const NetPlan& q = p.net[n]; const NetOff& o = w.net[q.type]; TrainBufs& t = w.tb[n];
        SeqFwdArgs fa{t.G[l], params + o.w_hh[l], t.Hm[l], t.Cm[l], t.Hout[l], t.TanhC[l], w.keep, w.seq_counters + SEQ_COUNTER_WORDS * (4 * l + n), w.seq_err, T, B, (n == stamp_net && l == stamp_layer) ? w.seq_stamps : nullptr};
        if (q.fwd_folded0 && l == 0) {
          if (p.fuse_obs) { fa.X = t.obs; fa.ldx = o.ld_obs; fa.Wih = w.Weff; fa.ldw = o.ld_obs; fa.bias = w.beff; fa.kx = o.nin; }   // gates_0 = obs Weff^T + beff inside the recurrence
        } else if (p.fuse_ih) {   // K = H input projections ride inside the recurrence (kbj_lstm_seq.h FUSE)
          fa.X = l == 0 ? t.X0 : t.Hout[l - 1]; fa.Wih = params + o.w_ih[l]; fa.bias = params + o.b[l];
        }
        if (seq_fwd(ctx, q.lane, H, fa)) return -1;
      }
    }
    // both lanes wait for the side-lane gathers / clears (gathers): the actor's for ev_small, the critic's for its gathered rows (read by its
    // backward pass) - an event that implies ev_small - or ev_small itself
    return p.two_lanes && (ev_wait(ctx, p.net[0].lane, ctx->ev_small) || ev_wait(ctx, p.net[1].lane, p.gather_late ? ctx->ev_obs : ctx->ev_small)) ? -1 : 0;
  }

  // phase: heads forward - the output projections of the first `nets` nets (not the critic's when the fused head computes it with the loss),
  // then the actor's head: pre-activation, low-pass scan over time, log-probabilities and entropy. The critic's value is the caller's next launch.
  void heads_forward(int nets, float* logp, float* ent) {
    const hipStream_t s = p.net[0].lane;
    for (int n = 0; n < nets; ++n) {
      const NetOff& o = w.net[p.net[n].type];
      if (!(n == 1 && grad && p.fused_critic_head)) linear_fwd(p.net[n].lane, w.tb[n].Hout[D - 1], H, params + o.w_out, H, params + o.b_out, w.tb[n].Out, 40, R, o.nout, H, 0);
    }
    actor_head_pre_launch(s, w.tb[0].Out, w.tb[0].obs, w.joint_bias_d, hp, R, w.y, w.sd);
    actor_head_train_fwd_launch(s, w.keep, w.lpf0, hp, T, B, w.y);
    gaussian_logp_launch(s, w.y, w.sd, w.act, R, logp, ent);
  }

  // phase: losses. The policy terms need the actor only, the value terms the critic only (the mirror terms likewise), so each lane
  // computes its own and the two chains stay independent through the whole call: the shorter actor chain runs ahead, and its
  // recurrences meet the critic's GEMM phases instead of the critic's recurrences
  int losses() {
    const hipStream_t s = p.net[0].lane, sv = p.net[1].lane;   // the actor's lane, the critic's
    ppo_loss_launch(s, w.logp, w.value, w.ent, w.logp_old, w.val_old, w.adv, w.target, w.stats, pp, R, w.dlogp, w.dvalue, w.stats + 2, p.two_lanes ? 1 : 0);
    if (p.fused_critic_head) {
      const NetOff& oc = w.net[1]; TrainBufs& tc = w.tb[1];
      const bool built = critic_head_launch(sv, H, tc.Hout[D - 1], params + oc.w_out, params + oc.b_out, w.val_old, w.target, pp, R, w.value, w.dvalue, tc.dOut, tc.dHa, w.stats + 2);
      if (!built) return kbj_fail(ctx, "kbj_ppo_grad: critic_head_kernel is built for hidden sizes 64, 128, ..., 512");
      if (!p.two_lanes) ppo_loss_launch(s, w.logp, w.value, w.ent, w.logp_old, w.val_old, w.adv, w.target, w.stats, pp, R, w.dlogp, w.dvalue, w.stats + 2, 1);   // (the actor's launch above was a no-op in this diagnostic mode)
    } else {
      critic_value_launch(sv, w.tb[1].Out, 40, R, w.value);
      ppo_loss_launch(sv, w.logp, w.value, w.ent, w.logp_old, w.val_old, w.adv, w.target, w.stats, pp, R, w.dlogp, w.dvalue, w.stats + 2, p.two_lanes ? 2 : 3);
    }
    if (w.mirror) {   // aux losses between each net and its mirror branch (train.py:1463-1481)
      actor_head_pre_launch(s, w.tb[2].Out, w.tb[2].obs, w.joint_bias_d, hp, R, w.y_m, w.sd_m);
      actor_head_train_fwd_launch(s, w.keep, w.lpf0_m, hp, T, B, w.y_m);
      mirror_loss_launch(s, w.y, w.y_m, w.value, w.value_m, c.actor_mirror_loss_scale, c.critic_mirror_loss_scale, R, w.dy, w.dy_m, w.dvalue, w.dvalue_m, w.stats + 2, p.two_lanes ? 1 : 0);
      critic_value_launch(sv, w.tb[3].Out, 40, R, w.value_m);
      mirror_loss_launch(sv, w.y, w.y_m, w.value, w.value_m, c.actor_mirror_loss_scale, c.critic_mirror_loss_scale, R, w.dy, w.dy_m, w.dvalue, w.dvalue_m, w.stats + 2, p.two_lanes ? 2 : 3);
    }
    return p.two_lanes ? ev_record(ctx, p.ev_critic_loss, sv) : 0;   // for the metrics launch (UpdatePlan::ev_critic_loss)
  }

  // The two dH buffers of a net alternate down the layers: dh_of(t, l) is what layer l's backward recurrence reads (l = D - 1: the head's
  // input gradient), dh_of(t, l - 1) where its input gradient goes (l = 0: dX0, the input projection's)
  float* dh_of(const TrainBufs& t, int l) const { return (D - 1 - l) % 2 == 0 ? t.dHa : t.dHb; }

  // phase: head backward and output-projection gradients (dOut needs no clearing: the actor head writes all 40 columns, the critic's GEMMs read column 0 only)
  int heads_backward() {
    const hipStream_t s = p.net[0].lane;
    actor_head_bwd_pre_launch(s, w.tb[0].Out, w.y, w.sd, w.act, w.dlogp, w.mirror ? w.dy : (const float*)nullptr, -c.entropy_coef / (float)R, hp, R, w.tb[0].dOut);
    actor_head_train_bwd_launch(s, w.keep, hp, T, B, w.tb[0].dOut);
    if (!p.fused_critic_head) KBJ_HIP(ctx, hipMemcpy2DAsync(w.tb[1].dOut, 40 * sizeof(float), w.dvalue, sizeof(float), sizeof(float), R, hipMemcpyDeviceToDevice, p.net[1].lane));
    if (w.mirror) {   // the mirror actor only sees the aux gradient on its filtered mean (no log-prob, no entropy term)
      actor_head_bwd_pre_launch(s, w.tb[2].Out, w.y_m, w.sd_m, w.y_m, w.zeroR, w.dy_m, 0.0f, hp, R, w.tb[2].dOut);
      actor_head_train_bwd_launch(s, w.keep, hp, T, B, w.tb[2].dOut);
      KBJ_HIP(ctx, hipMemcpy2DAsync(w.tb[3].dOut, 40 * sizeof(float), w.dvalue_m, sizeof(float), sizeof(float), R, hipMemcpyDeviceToDevice, p.net[1].lane));
    }
    // The critical path of a net is dOut -> dH -> (recurrence, dX) per layer. Weight/bias gradients hang off it: they go to the
    // net's side lane so the throughput-bound split-K GEMMs run beside the dX GEMMs in the GEMM phases.
    for (int n = 0; n < p.nnets; ++n) {
      const NetPlan& q = p.net[n]; const NetOff& o = w.net[q.type]; TrainBufs& t = w.tb[n];
      if (!(n == 1 && p.fused_critic_head)) linear_bwd_input(q.lane, sc.gemm_x3, t.dOut, 40, params + o.w_out, H, t.dHa, H, R, H, o.nout, 0);
      if (n == 1 && p.critic_fork_recorded) { if (ev_wait(ctx, q.side, ctx->ev_side[1])) return -1; }   // recorded behind the loss (losses): one packet
      else if (fork_side(ctx, p, q)) return -1;
      linear_bwd_weight(ctx, q.side, sc.gemm_x3, t.dOut, 40, t.Hout[D - 1], H, grad + o.w_out, H, o.nout, H, R);
      colsum_acc(ctx, q.side, t.dOut, R, o.nout, 40, grad + o.b_out);
    }
    return 0;
  }

  // the bias terms of layer 0 of a folded net type k (db_0 is complete with the net's layer-0 recurrence; the read-modify-write of dW_ih0 must follow the
  // folded product into it, on the same lane): db_in = W_ih0^T db_0, dW_ih0 += db_0 b_in^T   (X0 = obs W_in^T + b_in)
  void fold_bias_terms(int k, hipStream_t st) {
    const NetOff& oa = w.net[k];
    float* part = det_partials(ctx, st);
    matvec_t_acc_launch(st, params + oa.w_ih[0], grad + oa.b[0], 4 * H, H, grad + oa.b_in, part);
    if (part) reduce_rows_launch(st, part, MATVEC_T_SLICES, H, grad + oa.b_in);
    outer_acc_launch(st, grad + oa.w_ih[0], grad + oa.b[0], params + oa.b_in, 4 * H, H);
  }

  // WHERE A LAYER'S WEIGHT-GRADIENT PAIR RUNS (round 6: explicit stream order, no pause kernel). The input gradient of layer l is on the
  // net's critical chain (the recurrence of layer l - 1 reads it) and the recurrences take whole CUs (250 registers x 2 wavefronts per SIMD):
  // a weight-gradient GEMM that is eligible at the same moment as a recurrence races it for the CUs, and a recurrence advances at the pace of
  // its last workgroup to be placed (+4 % per iteration when that race is lost). So the pair of layer l > 0 is ORDERED BEHIND THE END of the
  // net's layer l - 1 recurrence: on the net's own lane behind its layer-0 work when l - 1 is the last layer (nothing else is left for that
  // lane to do, and a cross-lane hop costs 15-20 us each way), else on the net's side lane behind an event recorded after the recurrence
  // launch. Rounds 4-5 reached the same order through a 30 us sleep kernel that in practice waited for a wave slot until the recurrences
  // retired (KBJ_DW_DELAY_US, seq_delay_kernel: deleted) - an accident of occupancy, not an order. No launch's start depends on another
  // launch's occupancy any more.
  void dw_pair(hipStream_t st, int n, int l) {
    const NetOff& o = w.net[p.net[n].type]; TrainBufs& t = w.tb[n];
    linear_bwd_weight2(ctx, st, sc.gemm_x3, t.dGl[l], 4 * H, t.Hm[l], l == 0 ? t.X0 : t.Hout[l - 1], H, grad + o.w_hh[l], grad + o.w_ih[l], H, 4 * H, H, R);
  }
  // the pair of layer l + 1 of net n, in pass l of the layer loop: ONE decision per net, asked at the two places of the pass where the pair
  // may be issued - right behind the pass's recurrence launches (at_tail = false) and last in the net's layer-0 work (at_tail = true)
  int dw_pair_above(int n, int l, bool at_tail) {
    const NetPlan& q = p.net[n];
    const bool on_tail = p.two_lanes && q.tail_on_lane && l == 0;   // last on the net's own lane (two lanes in the tail instead of four: measured equal)
    if (l + 1 >= D || on_tail != at_tail) return 0;
    if (!p.two_lanes || on_tail) { dw_pair(q.lane, n, l + 1); return 0; }   // (one lane: stream order is the order)
    if (hop(ctx, q.lane, q.side, ctx->ev_dx[q.type])) return -1;   // the side lane, behind the recurrence launch(es) of this pass on the net's lane
    dw_pair(q.side, n, l + 1);
    return 0;
  }

  // phase: one backward layer pass - the recurrences of layer l of every net, the weight-gradient pairs of layer l + 1, then per net the
  // input gradient (the next pass's dH) or, at a folded layer 0, the folded products
  // INVARIANT of the schedule: no kernel waits for another LAUNCH. The only inter-workgroup waits are those of the persistent recurrences,
  // inside one launch whose grid is resident by construction (kbj_nn_create). Everything else is ordered by stream events, so any
  // serialisation of kernels (rocprofv3 --pmc, AMD_SERIALIZE_KERNEL=3) runs the same schedule to the same results. (Round 3 / 4 carried
  // chunk-gated variants - a one-wavefront gate kernel polling a recurrence's progress in front of the GEMMs that consume it, KBJ_BWD_CHUNKS /
  // KBJ_DW_GATE: measured flat to 0.3 %, and dispatched alone under a serialising profiler the gate spins to its bound. They are gone,
  // DESIGN.md section 10.)
  int backward_layer(int l) {
    for (int n = 0; n < p.nnets; ++n) {
      const NetPlan& q = p.net[n]; const NetOff& o = w.net[q.type]; TrainBufs& t = w.tb[n];
      SeqBwdArgs ba{t.G[l], t.TanhC[l], t.Cm[l], dh_of(t, l), w.keep, params + o.w_hh[l], t.dGl[l], w.seq_counters + SEQ_COUNTER_WORDS * (4 * (D + l) + n), w.seq_err, T, B, grad + o.b[l]};
      ba.db_part = det_partials(ctx, q.lane);   // deterministic mode: per-row-group bias sums, added in order below
      if (w.seq_bstamps && ctx->set.bstamp_sel == 1 + n + 2 * l) ba.stamps = w.seq_bstamps;   // diagnostics build only
      if (seq_bwd(ctx, q.lane, H, ba, sc.bwd16)) return -1;
      if (ba.db_part) reduce_rows_launch(q.lane, ba.db_part, seq_bwd_row_groups(B, sc.bwd16), 4 * H, grad + o.b[l]);
    }
    // the layer above's weight gradients, behind THIS layer's recurrence of the same net
    for (int n = 0; n < p.nnets; ++n)
      if (dw_pair_above(n, l, false)) return -1;
    for (int n = 0; n < p.nnets; ++n) {
      const NetPlan& q = p.net[n]; const NetOff& o = w.net[q.type]; TrainBufs& t = w.tb[n];
      if (!(q.folded0 && l == 0)) {
        // the input gradient as ONE product on the net's own lane, behind the recurrence (it is the next layer's input)
        linear_bwd_input(q.lane, sc.gemm_x3, t.dGl[l], 4 * H, params + o.w_ih[l], H, dh_of(t, l - 1), H, R, H, 4 * H, 0, H <= 256 ? 2 : -1);
        // the weight gradients: in the next pass, behind layer l - 1's recurrence (dw_pair_above); layer 0's start behind the input gradient
        if (l == 0 && fork_side(ctx, p, q)) return -1;
        if (l == 0) dw_pair(q.side, n, 0);
        continue;
      }
      const hipStream_t ws = q.tail_on_lane ? q.lane : q.side;   // (NetPlan::tail_on_lane)
      if (!q.tail_on_lane && fork_side(ctx, p, q)) return -1;     // the side lane starts behind the whole recurrence
      // layer 0 backwards through the (activation-free) input projection without dX0: dW_hh0 += dG0^T Hm and Z = dG0^T obs in
      // one launch; two small products then carry Z back to the stored parameters
      float* Z = w.Zeff[n];
      const int ts = H % 128 == 0 ? 128 : 64;   // the column split (n1 = H) must fall on a tile boundary
      int sk = std::max(2, std::min(g_splitk_wgs / ((4 * H / ts) * (H / ts + (o.nin + ts - 1) / ts)), (R + 255) / 256));
      GemmArgs g{t.dGl[0], t.Hm[0], grad + o.w_hh[0], nullptr, 4 * H, H + o.nin, R, 4 * H, H, H, 1, sk, nullptr};
      g.B2 = t.obs; g.C2 = Z; g.n1 = H; g.ldb2 = o.ld_obs; g.ldc2 = o.ld_obs;
      g.skws = sk_workspace(ctx, ws, (size_t)sk * 4 * H * (H + o.nin));
      g.x3 = sc.gemm_x3;
      gemm_launch<false, false>(ws, g, ts == 128 ? 1 : 0);
      // dW_in += W_ih0^T Z, dW_ih0 += Z W_in^T (the bias terms follow from db_0 at the end)
      // (a 4H-deep contraction on a handful of output tiles: split over k so that it is a short kernel, not a 130 us tail on 32 workgroups)
      GemmArgs g1a{params + o.w_ih[0], Z, grad + o.w_in, nullptr, H, o.nin, 4 * H, H, o.ld_obs, o.nin, 1, g_fold_sk, nullptr};
      g1a.skws = sk_workspace(ctx, ws, (size_t)g_fold_sk * H * o.nin);   // (same lane, stream-ordered behind the launch above: the slab is free again)
      gemm_launch<false, false>(ws, g1a);
      GemmArgs g2a{Z, params + o.w_in, grad + o.w_ih[0], nullptr, 4 * H, H, o.nin, o.ld_obs, o.nin, H, 1, 1, nullptr};
      gemm_launch<true, true>(ws, g2a);
      // (365.3 / 364.5 / 363.6 -> 364.8 / 363.8 / 362.9 ms per iteration: the critic's pair no longer waits for the last low-priority GEMM)
      if (q.tail_on_lane && n < 2) { fold_bias_terms(n, ws); bias_done[n] = true; }   // right here, on the net's own lane: not behind the side lane's join at the end
      if (dw_pair_above(n, l, true)) return -1;
    }
    return 0;
  }

  // phase: input-projection gradients of the nets that are not folded, and the joins of the side lanes
  int projection_grads_and_joins() {
    for (int n = 0; n < p.nnets; ++n) {
      const NetPlan& q = p.net[n]; const NetOff& o = w.net[q.type]; TrainBufs& t = w.tb[n];
      if (!q.folded0) {   // input projection (dX0: where layer 0's input gradient went)
        linear_bwd_weight(ctx, q.lane, sc.gemm_x3, dh_of(t, -1), H, t.obs, o.ld_obs, grad + o.w_in, o.nin, H, o.nin, R);
        colsum_acc(ctx, q.lane, dh_of(t, -1), R, H, H, grad + o.b_in);
      }
      if (!p.two_lanes) continue;
      // join of the net's side lane (output-projection gradients, bias sums). The critic's side lane joins the ACTOR's lane when nothing on the
      // critic's own lane reads what it wrote any more (bias terms done): the actor's lane is joined into the caller's stream below, so the
      // critic's chain - on the caller's stream by default - ends with ONE event wait, for an event that fired long before
      const bool to_actor = q.type == 1 && q.lane == ctx->stream && bias_done[1];
      if (hop(ctx, q.side, to_actor ? p.net[0].lane : q.lane, ctx->ev_side[q.type])) return -1;
    }
    return 0;
  }

  // phase: lane tails.
  // Each lane ends with ONE small kernel behind its last gradient GEMM: it clears the hand-off counter blocks of the lane's nets (every recurrence
  // of the call has run: the next kbj_ppo_grad / kbj_ppo_forward starts without a clear on its chain) and poisons the lane's slice of the gradient
  // when a recurrence timed out (a truncated gradient: every data-parallel rank must skip the optimizer step; one NaN marker per slice is
  // enough, the norm covers the whole vector).
  // The actor's slice grad[0, nactor) is final here, ~0.4 ms before the critic's (shorter chain: folded layer 0, no 475-wide projection).
  // A data-parallel host may start its all-reduce now, under the critic's tail (kbj_stream_wait_actor_grad).
  int lane_tails(float* metrics_d) {
    const hipStream_t sa = p.net[0].lane, sv = p.net[1].lane;   // the actor's lane, the critic's
    if (p.net[0].folded0 && !bias_done[0]) fold_bias_terms(0, sa);
    if (p.two_lanes && ev_wait(ctx, sa, p.ev_critic_loss)) return -1;   // (UpdatePlan::ev_critic_loss says what this waits for in each case)
    ppo_metrics_launch(sa, w.stats + 2, w.stats, pp, R, metrics_d);
    if (!p.two_lanes) {
      if (p.net[1].folded0 && !bias_done[1]) fold_bias_terms(1, sv);
      hipLaunchKernelGGL(lane_tail_kernel, dim3(2 * MAXD * 4), dim3(SEQ_COUNTER_WORDS), 0, ctx->stream, w.seq_counters, -1, w.seq_err, grad, grad + w.nactor);
      return ev_record(ctx, ctx->ev_actor_grad, ctx->stream);
    }
    hipLaunchKernelGGL(lane_tail_kernel, dim3(2 * MAXD * 4), dim3(SEQ_COUNTER_WORDS), 0, sa, w.seq_counters, 0, w.seq_err, grad, (float*)nullptr);
    if (ev_record(ctx, ctx->ev_actor_grad, sa)) return -1;
    if (p.net[1].folded0 && !bias_done[1]) fold_bias_terms(1, sv);   // on the critic's own lane (its side lane has joined it above), beside the actor's
    hipLaunchKernelGGL(lane_tail_kernel, dim3(2 * MAXD * 4), dim3(SEQ_COUNTER_WORDS), 0, sv, w.seq_counters, 1, w.seq_err, grad + w.nactor, (float*)nullptr);
    // join: the lane that is NOT the caller's stream into the caller's stream. With the critic on the caller's stream (default) the wait is for an
    // event that was recorded long ago - the actor's lane finishes first - so the tail of a minibatch crosses no queue either.
    return hop(ctx, ctx->stream2, ctx->stream, ctx->ev_join);
  }
};

int ppo_forward_body(kbj_ctx* ctx, const float* params_d, const kbj_traj* tr, const int32_t* env_idx_d, kbj_ppo_vars* out) {
  Update u{ctx, params_d, tr, env_idx_d, nullptr, nullptr, nullptr};
  NnWs& w = u.w;
  const hipStream_t s = u.p.net[0].lane;   // the actor's lane
  if (u.lanes_begin() || u.folded_weights() || u.gathers() || u.input_projections() || u.forward_recurrences()) return -1;
  u.heads_forward(2, out->logp_d, out->entropy_d ? out->entropy_d : w.ent);
  if (out->action_std_d) KBJ_HIP(ctx, hipMemcpyAsync(out->action_std_d, w.sd, (size_t)u.R * KBJ_NU * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (out->action_mean_d) KBJ_HIP(ctx, hipMemcpyAsync(out->action_mean_d, w.y, (size_t)u.R * KBJ_NU * sizeof(float), hipMemcpyDeviceToDevice, s));
  critic_value_launch(u.p.net[1].lane, w.tb[1].Out, 40, u.R, out->value_d);
  if (u.p.two_lanes && hop(ctx, ctx->stream2, ctx->stream, ctx->ev_join)) return -1;
  hipLaunchKernelGGL(poison_vars_kernel, dim3(1), dim3(1), 0, ctx->stream, w.seq_err, out->logp_d, out->value_d);   // a recurrence timed out: no silent garbage
  KBJ_CHECK_LAUNCH(ctx, "kbj_ppo_forward");
  if (u.sc.debug_sync) return kbj_synchronize(ctx);
  return 0;
}

int ppo_grad_body(kbj_ctx* ctx, const float* params_d, const kbj_traj* tr, const int32_t* env_idx_d, const float* adv_d, const float* target_d,
                  float* grad_d, float* metrics_d) {
  KbjTimed timed(ctx, true);
  Update u{ctx, params_d, tr, env_idx_d, adv_d, target_d, grad_d};
  if (u.lanes_begin() || u.folded_weights() || u.gathers() || u.input_projections() || u.forward_recurrences()) return -1;
  u.heads_forward(u.p.nnets, u.w.logp, u.w.ent);
  if (u.losses() || u.heads_backward()) return -1;
  for (int l = u.D - 1; l >= 0; --l)
    if (u.backward_layer(l)) return -1;
  if (u.projection_grads_and_joins() || u.lane_tails(metrics_d)) return -1;
#ifndef KBJ_NO_TAIL_CLEAN   // A/B
  u.w.counters_clean = true;
#endif
  KBJ_CHECK_LAUNCH(ctx, "kbj_ppo_grad");
  if (u.sc.debug_sync) return kbj_synchronize(ctx);   // KBJ_DEBUG=1: surface a hand-off timeout at the call that caused it
  return 0;
}

}  // namespace

extern "C" {

int kbj_ppo_forward(kbj_ctx* ctx, const float* params_d, const kbj_traj* tr, const int32_t* env_idx_d, int B, kbj_ppo_vars* out) {
  if (!ctx || !params_d || !tr || !env_idx_d || !out || !out->logp_d || !out->value_d) return kbj_fail(ctx, "kbj_ppo_forward: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  if (B != w.B) return kbj_fail(ctx, "kbj_ppo_forward: B must equal config.batch_size");
  if (tr->T != w.T || tr->N != w.N) return kbj_fail(ctx, "kbj_ppo_forward: trajectory shape does not match the context");
  if (!w.padded()) return ppo_forward_body(ctx, params_d, tr, env_idx_d, out);
  pad_params(ctx, ctx->stream, params_d, w.pparams);
  kbj_traj pt = pad_traj_carry0(ctx, ctx->stream, *tr);
  return ppo_forward_body(ctx, w.pparams, &pt, env_idx_d, out);
}

int kbj_ppo_grad(kbj_ctx* ctx, const float* params_d, const kbj_traj* tr, const int32_t* env_idx_d, int B, const float* adv_d, const float* target_d,
                 float* grad_d, float* metrics_d) {
  if (!ctx || !params_d || !tr || !env_idx_d || !adv_d || !target_d || !grad_d || !metrics_d) return kbj_fail(ctx, "kbj_ppo_grad: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  if (B != w.B) return kbj_fail(ctx, "kbj_ppo_grad: B must equal config.batch_size");
  if (tr->T != w.T || tr->N != w.N) return kbj_fail(ctx, "kbj_ppo_grad: trajectory shape does not match the context");
  if (!w.padded()) return ppo_grad_body(ctx, params_d, tr, env_idx_d, adv_d, target_d, grad_d, metrics_d);
  hipStream_t s = ctx->stream;
  pad_params(ctx, s, params_d, w.pparams);
  kbj_traj pt = pad_traj_carry0(ctx, s, *tr);
  const int rc = ppo_grad_body(ctx, w.pparams, &pt, env_idx_d, adv_d, target_d, w.pgrad, metrics_d);
  if (rc) return rc;
  unpad_params(ctx, s, w.pgrad, grad_d);          // the poison markers of a timed-out recurrence sit on real elements: they travel
  KBJ_HIP(ctx, hipEventRecord(ctx->ev_actor_grad, s));   // the caller's actor slice is final only now
  KBJ_CHECK_LAUNCH(ctx, "pad_params_kernel");
  return 0;
}

int kbj_ppo_prefetch(kbj_ctx* ctx, const kbj_traj* traj, const int32_t* env_idx_d) {
  if (!ctx || !ctx->nn_ws || !traj || !env_idx_d) return kbj_fail(ctx, "kbj_ppo_prefetch: null argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  if (traj->T != w.T || traj->N != w.N) return kbj_fail(ctx, "kbj_ppo_prefetch: trajectory shape does not match the context");
  if (w.sched.one_stream || w.padded()) return 0;      // nothing to overlap with on one lane; padded sizes re-pitch the carries per call: served without the hint
  hipStream_t lane = ctx->side[1];
  if (hop(ctx, ctx->stream, lane, ctx->ev_fork)) return -1;      // behind everything queued so far (the previous minibatch's last reader of these buffers)
  if (head_gathers(ctx, lane, traj, env_idx_d) || ev_record(ctx, ctx->ev_prefetch, lane)) return -1;
  w.prefetched_idx = env_idx_d; w.prefetched_traj = traj;
  KBJ_CHECK_LAUNCH(ctx, "kbj_ppo_prefetch");
  return 0;
}

int kbj_recurrence_residency(kbj_ctx* ctx, int* grid_wgs, int* concurrent, int* slots) {
  if (!ctx || !ctx->nn_ws || !grid_wgs || !concurrent || !slots) return kbj_fail(ctx, "kbj_recurrence_residency: null argument");
  const NnWs& w = *ws_of(ctx);
  *grid_wgs = w.seq_grid; *concurrent = w.sched.one_stream ? 1 : 2; *slots = w.seq_slots;
  return 0;
}

int kbj_set_rollout_argmax(kbj_ctx* ctx, int argmax) {
  if (!ctx) return kbj_fail(nullptr, "kbj_set_rollout_argmax: null ctx");
  ctx->rollout_argmax = argmax != 0;
  return 0;
}

int kbj_set_advantage_sums(kbj_ctx* ctx, const double* sums_d) {
  if (!ctx || !ctx->nn_ws) return kbj_fail(ctx, "kbj_set_advantage_sums: null ctx");
  ws_of(ctx)->ext_adv_sums = sums_d;
  return 0;
}

int kbj_stream_wait_actor_grad(kbj_ctx* ctx, void* hip_stream) {
  if (!ctx) return kbj_fail(nullptr, "kbj_stream_wait_actor_grad: null ctx");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  KBJ_HIP(ctx, hipStreamWaitEvent((hipStream_t)hip_stream, ctx->ev_actor_grad, 0));
  return 0;
}

int kbj_set_learning_rate(kbj_ctx* ctx, float learning_rate) {
  // a negative rate is legal: the reference's scale_by_adam + scale_by_schedule chain (train.py:1074-1075) has no sign flip and is served
  // as written by passing minus the schedule's value (host/task.py update())
  if (!ctx || !std::isfinite(learning_rate)) return kbj_fail(ctx, "kbj_set_learning_rate: bad argument");
  ctx->cfg_h.learning_rate = learning_rate;
  return 0;
}

int kbj_adamw_step(kbj_ctx* ctx, float* params_d, float* m_d, float* v_d, const float* grad_d, int64_t step, float grad_scale) {
  if (!ctx || !params_d || !m_d || !v_d || !grad_d || step < 1) return kbj_fail(ctx, "kbj_adamw_step: bad argument");
  KBJ_HIP(ctx, hipSetDevice(ctx->device));
  NnWs& w = *ws_of(ctx);
  const kbj_config& c = ctx->cfg_h;
  hipStream_t s = ctx->stream;
  double* sumsq = w.stats + 10;
  // one launch less on the chain between the last gradient GEMM and the next minibatch's first kernel: the accumulator is already zero when this
  // step follows a kbj_ppo_grad (whose clear of the statistics block covers it); any other caller (several steps in a row, per-pass accumulation) clears it here
  if (!w.sumsq_clean) KBJ_HIP(ctx, hipMemsetAsync(sumsq, 0, sizeof(double), s));
  w.sumsq_clean = false;
  double* part = w.sched.deterministic ? w.detd : nullptr;
  sumsq_launch(s, grad_d, w.user.nparams, grad_scale, sumsq, part);
  if (part) reduce_double_launch(s, part, SUMSQ_BLOCKS, 1, sumsq);
  AdamParams ap{c.learning_rate, c.adam_b1, c.adam_b2, c.adam_eps, c.weight_decay, c.max_grad_norm,
                (float)(1.0 - std::pow((double)c.adam_b1, (double)step)), (float)(1.0 - std::pow((double)c.adam_b2, (double)step)), grad_scale};
  hipLaunchKernelGGL(adamw_kernel, g1(w.user.nparams), dim3(256), 0, s, params_d, m_d, v_d, grad_d, w.user.nparams, sumsq, ap, w.seq_err);
  KBJ_CHECK_LAUNCH(ctx, "adamw_kernel");
  return 0;
}

}  // extern "C"
