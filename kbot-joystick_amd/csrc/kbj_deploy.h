// kbj_deploy.h — the deployed actor step: convert.py's step_fn (convert.py:85-119) as ONE launch, one 256-thread workgroup per row.
//
// What the robot runs is step_fn(joint_angles, joint_angular_velocities, projected_gravity, gyroscope, command, carry) -> (action, carry)
// with one flat carry per row (ravel_pytree(Carry(actor_carry [depth][2][H], lpf [20])), convert.py:74-78): per layer h [H] then c [H], then
// the 20 low-pass floats. kbj_policy_step is the TRAINING path (packed rows, plane carries, critic, sampling, a chain of launches sized for
// thousands of rows); this is the latency path: matrix-vector products on the vector units, no MFMA, the parameters read in the caller's
// own layout (kbj.h leaf order at its real hidden_size: no padding, no re-pitched copy). H in 1..512 and depth in 1..4 are run-time values.
//
// Per row: pack the 65-float observation from the raw sensors (convert.py:93-105, train.py:1329-1349) -> input projection -> depth x
// (gates = W_ih x + W_hh h + b, cell) -> the 20 mean rows of the output projection -> + joint bias + arm command (train.py:932-933) ->
// one-pole low-pass (train.py:936). The action is the filtered mean (dist.mode(), convert.py:119) and IS the new low-pass state.
//
// Matrix-vector product: lanes run along k. Lane l owns the four consecutive k = 256 j + 4 l + (0..3) of every 256-float chunk j, so a
// wavefront reads a weight row as contiguous 1 KB segments (one float4 per lane; scalar loads of the same elements when H is no multiple of
// 4 or the parameter vector is not 16-byte aligned). A wavefront has DEPLOY_R rows in flight: with both matrices of a layer that is up to
// 32 independent 16-byte loads per lane before the first use, which is what covers the L2 latency when one workgroup is all there is.
// Each lane adds its products in ascending k into one accumulator (W_ih's, then W_hh's), the 64 partials go through the wave sum of
// kbj_wave.h (wsum2: two rows per tree), the bias is added last. The order depends on nothing but H, so a row's result is bitwise
// independent of N, of its position in the batch, of vector or scalar loads and of whether the carry is updated in place.
//
// A workgroup reads its WHOLE carry row into LDS before anything else and writes it back as its last act, so carry_out == carry_in is
// allowed. All stores are ordinary vector stores; no atomics, no flags, nothing waits on another workgroup. Every workgroup re-reads the
// actor's weights through L2: the design range is N <= 64 (larger N is correct, kbj_policy_step stays the throughput path).
// LDS (floats): packed row 68 | x H | gates 4 H | carry 2 depth H + 20: 9.6 KB at H = 256, depth 2; 27 KB at H = 512, depth 4.
#pragma once
#include <hip/hip_runtime.h>
#include "kbj.h"
#include "kbj_wave.h"          // wsum2
#include "kbj_obs_encode.h"    // encode_pg
#include "kbj_nn_kernels.h"    // lstm_cell_point

namespace kbj {

constexpr int DEPLOY_THREADS = 256, DEPLOY_WAVES = DEPLOY_THREADS / 64;
constexpr int DEPLOY_R = 8;    // rows one wavefront has in flight (even: wsum2 sums them in pairs)

struct DeployArgs {
  const float* params;         // the actor's leaves, caller's layout
  kbj_deploy_inputs in;
  const float* carry_in; float* carry_out; float* action;
  const kbj_model* model;      // joint_bias / joint_lo / joint_hi
  float alpha;
  int H, D;
  size_t w_in, b_in, w_ih[KBJ_MAX_DEPTH], w_hh[KBJ_MAX_DEPTH], b[KBJ_MAX_DEPTH], w_out, b_out;   // float offsets into params
};

__host__ __device__ inline int deploy_round4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int deploy_gate_floats(int H) { return 4 * H > KBJ_NU ? 4 * H : KBJ_NU; }   // the 20 output rows reuse the gates' place
inline size_t deploy_lds_bytes(int H, int D) { return sizeof(float) * (size_t)(KBJ_LD_ACTOR + deploy_round4(H) + deploy_gate_floats(H) + 2 * D * H + KBJ_NU); }

// this lane's share of one row: acc += sum over its k of w[k] x[k], ascending k. NCH = 256-float chunks of a row (K <= 256 NCH).
// Straight-line code: a lane whose k lies past the end of the row loads the row's last element(s) instead and drops the product with a
// select, so that no load sits behind a branch and all of a wavefront's rows are in flight together.
template <bool VEC, int NCH> struct DeployRow {
  float4 w[NCH];
  KBJ_DEV void load(const float* __restrict__ row, int K, int lane) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int k0 = 256 * j + 4 * lane;
      if (VEC) w[j] = *reinterpret_cast<const float4*>(row + min(k0, K - 4));   // K % 4 == 0
      else { w[j].x = row[min(k0 + 0, K - 1)]; w[j].y = row[min(k0 + 1, K - 1)]; w[j].z = row[min(k0 + 2, K - 1)]; w[j].w = row[min(k0 + 3, K - 1)]; }
    }
  }
  KBJ_DEV float dot(const float* x, int K, int lane, float acc) const {   // x: LDS
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int k0 = 256 * j + 4 * lane;
      float t;
      if (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(x + min(k0, K - 4));
        t = fmaf(w[j].x, v.x, acc); t = fmaf(w[j].y, v.y, t); t = fmaf(w[j].z, v.z, t); t = fmaf(w[j].w, v.w, t);
        acc = k0 < K ? t : acc;
      } else {
        t = fmaf(w[j].x, x[min(k0 + 0, K - 1)], acc); acc = k0 + 0 < K ? t : acc;
        t = fmaf(w[j].y, x[min(k0 + 1, K - 1)], acc); acc = k0 + 1 < K ? t : acc;
        t = fmaf(w[j].z, x[min(k0 + 2, K - 1)], acc); acc = k0 + 2 < K ? t : acc;
        t = fmaf(w[j].w, x[min(k0 + 3, K - 1)], acc); acc = k0 + 3 < K ? t : acc;
      }
    }
    return acc;
  }
};

// y[r] = (W1[r] . x1 + W2[r] . x2) + add[r] for r < nrows; W1, W2 row-major [nrows][K], x1, x2, y in LDS. Wavefront w takes the DEPLOY_R
// consecutive rows from (4 i + w) DEPLOY_R on; rows past the end are clamped to the last one and dropped, so every wavefront runs the
// reduction with all lanes enabled (the DPP forms of kbj_wave.h need that). The caller synchronises before y is read.
template <bool VEC, int NCH, bool TWO> KBJ_DEV void deploy_matvec(const float* __restrict__ W1, const float* x1, const float* __restrict__ W2, const float* x2, int K,
                                                                  const float* __restrict__ add, int nrows, float* y) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r0 = wave * DEPLOY_R; r0 < nrows; r0 += DEPLOY_WAVES * DEPLOY_R) {
    DeployRow<VEC, NCH> a[DEPLOY_R], b[TWO ? DEPLOY_R : 1];
#pragma unroll
    for (int i = 0; i < DEPLOY_R; ++i) {
      const size_t r = (size_t)min(r0 + i, nrows - 1);
      a[i].load(W1 + r * K, K, lane);
      if (TWO) b[i].load(W2 + r * K, K, lane);
    }
    const bool mine = lane < DEPLOY_R && r0 + lane < nrows;
    const float bias = mine ? add[r0 + lane] : 0.0f;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < DEPLOY_R; i += 2) {
      float p0 = a[i].dot(x1, K, lane, 0.0f), p1 = a[i + 1].dot(x1, K, lane, 0.0f);
      if (TWO) { p0 = b[i].dot(x2, K, lane, p0); p1 = b[i + 1].dot(x2, K, lane, p1); }
      float s0, s1;
      wsum2(p0, p1, s0, s1);
      s = lane == i ? s0 : (lane == i + 1 ? s1 : s);
    }
    if (mine) y[r0 + lane] = s + bias;
  }
}

template <bool VEC, int NCH> __global__ __launch_bounds__(DEPLOY_THREADS) void actor_deploy_step_kernel(DeployArgs a) {
  extern __shared__ float4 deploy_lds[];
  const int H = a.H, D = a.D, tid = threadIdx.x;
  const size_t n = blockIdx.x;
  const int ncarry = 2 * D * H + KBJ_NU;
  float* S_row = reinterpret_cast<float*>(deploy_lds);      // [68] packed observation (65 used)
  float* S_x = S_row + KBJ_LD_ACTOR;                        // [H] input projection
  float* S_g = S_x + deploy_round4(H);                      // [4 H] gate pre-activations; afterwards the 20 output rows
  float* S_c = S_g + deploy_gate_floats(H);                              // [depth][2][H] h, c and [20] low-pass: the row's flat carry
  const kbj_model& m = *a.model;

  // the whole carry row, before anything of it is written
  for (int k = tid; k < ncarry; k += DEPLOY_THREADS) S_c[k] = a.carry_in[n * ncarry + k];
  // pack the observation row (convert.py:93-105): the expressions of task_write_obs (kbj_env_task.h)
  if (tid < KBJ_NU) {
    const int u = tid;
    const float range = fmaxf(m.joint_bias[u] - m.joint_lo[u], m.joint_hi[u] - m.joint_bias[u]);
    S_row[KBJ_OBS_JPOS + u] = (a.in.joint_angles_d[n * KBJ_NU + u] - m.joint_bias[u]) / range;
    S_row[KBJ_OBS_JVEL + u] = a.in.joint_angular_velocities_d[n * KBJ_NU + u] / KBJ_OBS_JVEL_DIV;
  } else if (tid == 64) {
    float g[3], o[5];
    for (int k = 0; k < 3; ++k) g[k] = a.in.projected_gravity_d[n * 3 + k];
    encode_pg(g, o);
    for (int k = 0; k < 5; ++k) S_row[KBJ_OBS_PG + k] = o[k];
    for (int k = 0; k < 3; ++k) S_row[KBJ_OBS_GYRO + k] = a.in.gyroscope_d[n * 3 + k];
  } else if (tid >= 128 && tid < 128 + KBJ_NCMD) {
    const float* cmd = a.in.command_d + n * KBJ_NCMD;
    S_row[KBJ_OBS_CMD + tid - 128] = cmd[tid - 128];
    if (tid == 128) S_row[KBJ_OBS_ZEROCMD] = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1] + cmd[2] * cmd[2]) < 1e-3f ? 1.0f : 0.0f;
  }
  __syncthreads();

  const float* P = a.params;
  deploy_matvec<false, 1, false>(P + a.w_in, S_row, nullptr, nullptr, KBJ_NOBS_ACTOR, P + a.b_in, H, S_x);   // rows of 65 floats: never 16-byte aligned
  __syncthreads();
  const float* x = S_x;
  for (int l = 0; l < D; ++l) {
    float* h = S_c + 2 * l * H;
    float* c = h + H;
    deploy_matvec<VEC, NCH, true>(P + a.w_ih[l], x, P + a.w_hh[l], h, H, P + a.b[l], 4 * H, S_g);
    __syncthreads();
    for (int u = tid; u < H; u += DEPLOY_THREADS) {
      float gi, gf, gg, go, cn, tc;
      lstm_cell_point(S_g[u], S_g[H + u], S_g[2 * H + u], S_g[3 * H + u], c[u], gi, gf, gg, go, cn, tc);
      h[u] = go * tc;
      c[u] = cn;
    }
    __syncthreads();
    x = h;
  }
  deploy_matvec<VEC, NCH, false>(P + a.w_out, x, nullptr, nullptr, H, P + a.b_out, KBJ_NU, S_g);   // the 20 mean rows; the std head is not evaluated
  __syncthreads();
  if (tid < KBJ_NU) {   // train.py:932-936, the expressions of actor_head_lpf_kernel
    const int j = tid;
    const float mean = S_g[j] + m.joint_bias[j] + (j >= 10 ? S_row[KBJ_OBS_CMD + 6 + (j - 10)] : 0.0f);
    const float y0 = S_c[2 * D * H + j];
    const float y = y0 + a.alpha * (mean - y0);
    S_c[2 * D * H + j] = y;
    a.action[n * KBJ_NU + j] = y;
  }
  __syncthreads();
  for (int k = tid; k < ncarry; k += DEPLOY_THREADS) a.carry_out[n * ncarry + k] = S_c[k];
}

// N workgroups of 256 threads. vec: H % 4 == 0 and a 16-byte aligned parameter vector (every leaf of the actor then starts on 16 bytes)
inline void actor_deploy_step_launch(hipStream_t st, const DeployArgs& a, int N) {
  const bool vec = a.H % 4 == 0 && reinterpret_cast<uintptr_t>(a.params) % 16 == 0;
  const dim3 grid((unsigned)N), block(DEPLOY_THREADS);
  const size_t lds = deploy_lds_bytes(a.H, a.D);
  if (a.H <= 256) {
    if (vec) hipLaunchKernelGGL((actor_deploy_step_kernel<true, 1>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((actor_deploy_step_kernel<false, 1>), grid, block, lds, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((actor_deploy_step_kernel<true, 2>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((actor_deploy_step_kernel<false, 2>), grid, block, lds, st, a);
  }
}

}  // namespace kbj
