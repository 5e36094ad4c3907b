// kbj_terminal_value.h — the critic's value of the state an episode TIMED OUT in (kbj_critic_terminal_value; kbj_config.gae_terminal_value):
// ONE launch, one 256-thread workgroup per env row, and work only where a row needs it.
//
// A time-out is rare (about N / 600 rows per control step) but arrives all at once early in a run, and the terminal observation exists for
// the rows that ended only (the env kernel's terminal rows, kbj_env_step_terminal). A full-width critic step per control step would
// roughly double the critic's share of the rollout for a result that is thrown away on 599 rows of 600. So: a workgroup whose row did not
// time out (done <= 0: running, or failed - a failure bootstraps from nothing) writes 0.0f and leaves before it reads anything else; after
// every call value[0..N) is fully defined. A workgroup whose row timed out (done > 0) runs the critic's step for that one row - input
// projection of the terminal row, `depth` LSTM layers from the row's critic carry, the value head - as matrix-vector products on the
// vector units: the matvec of the deployed actor step (kbj_deploy.h deploy_matvec: lanes along k, DEPLOY_R rows of a wavefront in
// flight, the wave sums of kbj_wave.h), the cell of lstm_cell_point. Every such workgroup re-reads the critic's parameters through L2.
//
// Reads only: the carry [D][2][N][H] (the critic's after the policy step of step t, BEFORE the carry reset) and the terminal rows are not
// written; the new h of a layer lives in LDS and dies with the workgroup. H and D are run-time values, H in 1..512, and the kernel takes
// the carries and the parameters at whatever hidden size the caller holds them: kbj_rollout passes the kernels' (zero-padded) width with
// its internal copies, kbj_critic_terminal_value the caller's own. Lane l owns the same k of every row at every width, a padded k
// contributes fmaf(0, 0, acc) = acc, and vector and scalar loads add in the same order, so the two give the same bits.
// LDS (floats): terminal row ld | x H | h_prev H | h H | gates 4 H: 15 KB at H = 512 with 64 user columns.
#pragma once
#include <hip/hip_runtime.h>
#include "kbj.h"
#include "kbj_deploy.h"        // deploy_matvec, DEPLOY_THREADS, deploy_round4
#include "kbj_nn_kernels.h"    // lstm_cell_point

namespace kbj {

constexpr int TERMV_NIN_CH = 3;   // 256-float chunks of a terminal row: 475 + KBJ_MAX_EXTRA_OBS = 539 columns <= 768
static_assert(KBJ_NOBS_CRITIC + KBJ_MAX_EXTRA_OBS <= 256 * TERMV_NIN_CH, "the input projection's chunk count must cover the widest critic row");

struct TermValueArgs {
  const float* params;         // a parameter vector in the kbj.h layout at hidden size H
  const float* rows;           // [N][ld] terminal critic rows (only rows with done > 0 are read)
  const float* hc;             // [D][2][N][H] the critic's carry
  const float* done; int done_stride;
  float* value;                // [N]
  int N, H, D, nin, ld;
  size_t w_in, b_in, w_ih[KBJ_MAX_DEPTH], w_hh[KBJ_MAX_DEPTH], b[KBJ_MAX_DEPTH], w_out, b_out;   // float offsets of the critic's leaves in params
};

inline size_t termv_lds_bytes(int H, int ld) { return sizeof(float) * (size_t)(ld + 3 * deploy_round4(H) + 4 * H); }

template <bool VEC, int NCH> __global__ __launch_bounds__(DEPLOY_THREADS) void critic_terminal_value_kernel(TermValueArgs a) {
  extern __shared__ float4 termv_lds[];
  const int H = a.H, tid = threadIdx.x;
  const size_t n = blockIdx.x, N = (size_t)a.N;
  if (!(a.done[n * a.done_stride] > 0.0f)) {     // uniform over the workgroup: nothing else is read
    if (tid == 0) a.value[n] = 0.0f;
    return;
  }
  float* S_row = reinterpret_cast<float*>(termv_lds);     // [ld] the terminal row
  float* S_x = S_row + a.ld;                               // [H] input projection; then every second layer's output
  float* S_hp = S_x + deploy_round4(H);                    // [H] the layer's h from the carry
  float* S_h = S_hp + deploy_round4(H);                    // [H] the other layers' output
  float* S_g = S_h + deploy_round4(H);                     // [4 H] gate pre-activations; afterwards the value
  for (int k = tid; k < a.ld; k += DEPLOY_THREADS) S_row[k] = a.rows[n * a.ld + k];
  __syncthreads();
  const float* P = a.params;
  deploy_matvec<false, TERMV_NIN_CH, false>(P + a.w_in, S_row, nullptr, nullptr, a.nin, P + a.b_in, H, S_x);   // rows of 475 (+ user) floats: not 16-byte aligned
  const float* x = S_x;
  for (int l = 0; l < a.D; ++l) {
    const float* h_prev = a.hc + ((size_t)(2 * l) * N + n) * H;
    const float* c_prev = a.hc + ((size_t)(2 * l + 1) * N + n) * H;
    for (int u = tid; u < H; u += DEPLOY_THREADS) S_hp[u] = h_prev[u];
    __syncthreads();      // x (the projection or the layer below) and h_prev are in place
    deploy_matvec<VEC, NCH, true>(P + a.w_ih[l], x, P + a.w_hh[l], S_hp, H, P + a.b[l], 4 * H, S_g);
    __syncthreads();
    float* out = (l & 1) ? S_x : S_h;     // never the buffer this layer read its input from
    for (int u = tid; u < H; u += DEPLOY_THREADS) {
      float gi, gf, gg, go, cn, tc;
      lstm_cell_point(S_g[u], S_g[H + u], S_g[2 * H + u], S_g[3 * H + u], c_prev[u], gi, gf, gg, go, cn, tc);
      out[u] = go * tc;
    }
    x = out;
  }
  __syncthreads();
  deploy_matvec<VEC, NCH, false>(P + a.w_out, x, nullptr, nullptr, H, P + a.b_out, 1, S_g);   // Critic.forward's output projection (train.py:993-1004)
  __syncthreads();
  if (tid == 0) a.value[n] = S_g[0];
}

// N workgroups of 256 threads. vec: H % 4 == 0 and a 16-byte aligned parameter vector (every LSTM leaf and the output row then start on 16 bytes)
inline void critic_terminal_value_launch(hipStream_t st, const TermValueArgs& a) {
  const bool vec = a.H % 4 == 0 && reinterpret_cast<uintptr_t>(a.params) % 16 == 0;
  const dim3 grid((unsigned)a.N), block(DEPLOY_THREADS);
  const size_t lds = termv_lds_bytes(a.H, a.ld);
  if (a.H <= 256) {
    if (vec) hipLaunchKernelGGL((critic_terminal_value_kernel<true, 1>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((critic_terminal_value_kernel<false, 1>), grid, block, lds, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((critic_terminal_value_kernel<true, 2>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((critic_terminal_value_kernel<false, 2>), grid, block, lds, st, a);
  }
}

}  // namespace kbj
