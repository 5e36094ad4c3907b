// kbj_episode_stats.h — episode accounting over one trajectory (kbj_episode_stats): per-env running sums carried across rollouts
// (KBJ_EACC_*) and the statistics of the episodes that finished inside this trajectory (KBJ_EPST_*). Included by kbj_traj_stats.hip.
//
// The scan over t is serial per env by definition, and 8192 envs are only 128 wavefronts: one thread per env reading global memory
// would sit on 100 dependent load latencies. So one workgroup of four wavefronts owns 64 consecutive envs. Wavefronts 1-3 stage chunks
// of EPST_TC time steps into LDS (double buffered): for a fixed t the block's reward-term rows are 3 KB of contiguous floats = exactly
// one 16-byte load per staging thread, its rewards 256 contiguous bytes, its DONE flags one dword out of each 288-byte aux row; the three
// height columns are fetched only where DONE < 0. Wavefront 0 meanwhile runs the ordered scan of the previous chunk from LDS, one env
// per lane, plain fp32 adds in the order the ABI defines. The per-lane statistics are combined in lane order, the workgroup partials in
// block order by a second, single-workgroup kernel: doubles, fixed order, no atomics, so a call is bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "kbj_model.h"

namespace kbj {
namespace {

constexpr int EPST_ENVS = 64;       // envs per workgroup = lanes of the scanning wavefront
constexpr int EPST_THREADS = 256;   // wavefront 0 scans, wavefronts 1-3 stage
constexpr int EPST_TC = 8;          // time steps per staged chunk (two chunk images = 58 KB of LDS)
constexpr int EPST_LD = EPST_ENVS + 1;   // row stride of the transposed reward-term image: the staging writes (12 terms of one env from 3 neighbouring lanes) spread over the banks
static_assert(EPST_ENVS * KBJ_NREW == 4 * (EPST_THREADS - 64), "one 16-byte load per staging thread covers the block's reward-term rows of one time step");
static_assert(EPST_THREADS % KBJ_EPST_SIZE == 0 && KBJ_EACC_TERM + KBJ_NREW <= KBJ_EACC_SIZE && KBJ_EPST_TERM_SUM + KBJ_NREW <= KBJ_EPST_SIZE, "episode statistics layout");

struct EpstChunk {
  float rew[EPST_TC][EPST_ENVS];
  float kind[EPST_TC][EPST_ENVS];            // 0 running, else the KBJ_EPST_* slot of the termination cause
  float comps[EPST_TC][KBJ_NREW][EPST_LD];   // [t][term][env]: the scan reads lane-contiguous rows
};

// the slots of a KBJ_EPST vector (kbj_ordered_reduce.h): counts and sums, but for the extreme returns and the longest episode
struct EpstSlots {
  static constexpr int SIZE = KBJ_EPST_SIZE;
  static __device__ inline double identity(int j) { return j == KBJ_EPST_RETURN_MIN ? (double)INFINITY : j == KBJ_EPST_RETURN_MAX ? -(double)INFINITY : 0.0; }
  static __device__ inline double combine(int j, double a, double b) {
    if (j == KBJ_EPST_RETURN_MIN) return b < a ? b : a;
    if (j == KBJ_EPST_RETURN_MAX || j == KBJ_EPST_LENGTH_MAX) return b > a ? b : a;
    return a + b;
  }
};

// grid = ceil(N / 64) workgroups of 256 threads; part_out [gridDim.x][KBJ_EPST_SIZE]
__global__ __launch_bounds__(EPST_THREADS) void episode_stats_kernel(const float* __restrict__ aux, const float* __restrict__ reward, const float* __restrict__ comps, int T, int N,
                                                                      float unhealthy_z, float* __restrict__ acc, double* __restrict__ part_out) {
  __shared__ __align__(16) EpstChunk buf[2];
  static_assert(sizeof(buf) >= sizeof(double) * EPST_ENVS * KBJ_EPST_SIZE, "the lane partials reuse the chunk images");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int e0 = blockIdx.x * EPST_ENVS, nb = min(EPST_ENVS, N - e0);
  const int nchunk = (T + EPST_TC - 1) / EPST_TC;
  const bool live = wave == 0 && lane < nb;       // this thread scans env e0 + lane

  // scanner state: the env's accumulator row and the statistics of the episodes it finishes in this trajectory
  float ret = 0, len = 0, term[KBJ_NREW], spare[2] = {0, 0};
  int n_height = 0, n_other = 0, n_trunc = 0;
  double ret_sum = 0, ret_sq = 0, len_sum = 0, fail_len_sum = 0, term_sum[KBJ_NREW];
  float ret_min = INFINITY, ret_max = -INFINITY, len_max = 0;
#pragma unroll
  for (int k = 0; k < KBJ_NREW; ++k) { term[k] = 0; term_sum[k] = 0; }
  float4* row = reinterpret_cast<float4*>(acc + (size_t)(e0 + lane) * KBJ_EACC_SIZE);
  if (live) {
    const float4 a0 = row[0], a1 = row[1], a2 = row[2], a3 = row[3];
    ret = a0.x; len = a0.y;
    term[0] = a0.z; term[1] = a0.w; term[2] = a1.x; term[3] = a1.y; term[4] = a1.z; term[5] = a1.w;
    term[6] = a2.x; term[7] = a2.y; term[8] = a2.z; term[9] = a2.w; term[10] = a3.x; term[11] = a3.y;
    spare[0] = a3.z; spare[1] = a3.w;
  }

  for (int c = -1; c < nchunk; ++c) {
    if (wave == 0) {
      if (live && c >= 0) {      // ordered scan of chunk c
        const EpstChunk& B = buf[c & 1];
        const int tc = min(EPST_TC, T - c * EPST_TC);
        for (int tt = 0; tt < tc; ++tt) {
          ret += B.rew[tt][lane];
          len += 1.0f;
          if (comps) {
#pragma unroll
            for (int k = 0; k < KBJ_NREW; ++k) term[k] += B.comps[tt][k][lane];
          }
          const int kind = (int)B.kind[tt][lane];
          if (kind != 0) {       // the episode ends with this step: into the statistics, row back to zero
            n_height += kind == KBJ_EPST_FAIL_HEIGHT; n_other += kind == KBJ_EPST_FAIL_OTHER; n_trunc += kind == KBJ_EPST_TRUNCATED;
            ret_sum += (double)ret; ret_sq += (double)ret * (double)ret;
            ret_min = fminf(ret_min, ret); ret_max = fmaxf(ret_max, ret);
            len_sum += (double)len; len_max = fmaxf(len_max, len);
            if (kind != KBJ_EPST_TRUNCATED) fail_len_sum += (double)len;
#pragma unroll
            for (int k = 0; k < KBJ_NREW; ++k) { term_sum[k] += (double)term[k]; term[k] = 0; }
            ret = 0; len = 0;
          }
        }
      }
    } else if (c + 1 < nchunk) {   // stage chunk c + 1: every load of the chunk is issued before the first LDS write waits for one
      const int s = tid - 64, t0 = (c + 1) * EPST_TC;
      EpstChunk& B = buf[(c + 1) & 1];
      float4 v[EPST_TC];
      const bool cv = comps != nullptr && s * 4 < nb * KBJ_NREW;     // nb * 12 is a multiple of 4: a 16-byte piece is inside the block's rows or outside
#pragma unroll
      for (int tt = 0; tt < EPST_TC; ++tt)
        if (cv && t0 + tt < T) v[tt] = *reinterpret_cast<const float4*>(comps + ((size_t)(t0 + tt) * N + e0) * KBJ_NREW + s * 4);
      if (wave == 1) {
        float r[EPST_TC];
#pragma unroll
        for (int tt = 0; tt < EPST_TC; ++tt) r[tt] = (lane < nb && t0 + tt < T) ? reward[(size_t)(t0 + tt) * N + e0 + lane] : 0.0f;
#pragma unroll
        for (int tt = 0; tt < EPST_TC; ++tt) B.rew[tt][lane] = r[tt];
      } else if (wave == 2) {
        float d[EPST_TC];
#pragma unroll
        for (int tt = 0; tt < EPST_TC; ++tt) d[tt] = (lane < nb && t0 + tt < T) ? aux[((size_t)(t0 + tt) * N + e0 + lane) * KBJ_AUX_SIZE + KBJ_AUX_DONE] : 0.0f;
#pragma unroll
        for (int tt = 0; tt < EPST_TC; ++tt) {
          float kind = d[tt] > 0.0f ? (float)KBJ_EPST_TRUNCATED : 0.0f;
          if (d[tt] < 0.0f) {   // the env kernel's height termination, from its own operands (kbj_env_task.h task_step)
            const float* a = aux + ((size_t)(t0 + tt) * N + e0 + lane) * KBJ_AUX_SIZE;
            const float height = a[KBJ_AUX_BASEZ] - fminf(a[KBJ_AUX_LFZ], a[KBJ_AUX_RFZ]);
            kind = height < unhealthy_z ? (float)KBJ_EPST_FAIL_HEIGHT : (float)KBJ_EPST_FAIL_OTHER;
          }
          B.kind[tt][lane] = kind;
        }
      }
      if (cv) {
        const int env = s / 3, k0 = 4 * (s % 3);
#pragma unroll
        for (int tt = 0; tt < EPST_TC; ++tt)
          if (t0 + tt < T) { B.comps[tt][k0][env] = v[tt].x; B.comps[tt][k0 + 1][env] = v[tt].y; B.comps[tt][k0 + 2][env] = v[tt].z; B.comps[tt][k0 + 3][env] = v[tt].w; }
      }
    }
    __syncthreads();
  }

  if (live) {
    row[0] = make_float4(ret, len, term[0], term[1]); row[1] = make_float4(term[2], term[3], term[4], term[5]);
    row[2] = make_float4(term[6], term[7], term[8], term[9]); row[3] = make_float4(term[10], term[11], spare[0], spare[1]);
  }
  // lane partials -> LDS (the chunk images are free: the loop's last barrier is behind every read and write of them), then slot j in lane order
  double* lp = reinterpret_cast<double*>(&buf[0]);
  if (wave == 0) {
    double* p = lp + lane * KBJ_EPST_SIZE;
    for (int j = 0; j < KBJ_EPST_SIZE; ++j) p[j] = EpstSlots::identity(j);      // lanes beyond the last env contribute the identity
    p[KBJ_EPST_EPISODES] = (double)(n_height + n_other + n_trunc);
    p[KBJ_EPST_FAIL_HEIGHT] = (double)n_height; p[KBJ_EPST_FAIL_OTHER] = (double)n_other; p[KBJ_EPST_TRUNCATED] = (double)n_trunc;
    p[KBJ_EPST_RETURN_SUM] = ret_sum; p[KBJ_EPST_RETURN_SUMSQ] = ret_sq; p[KBJ_EPST_RETURN_MIN] = (double)ret_min; p[KBJ_EPST_RETURN_MAX] = (double)ret_max;
    p[KBJ_EPST_LENGTH_SUM] = len_sum; p[KBJ_EPST_LENGTH_MAX] = (double)len_max; p[KBJ_EPST_FAIL_LENGTH_SUM] = fail_len_sum;
#pragma unroll
    for (int k = 0; k < KBJ_NREW; ++k) p[KBJ_EPST_TERM_SUM + k] = term_sum[k];
  }
  __syncthreads();
  if (tid < KBJ_EPST_SIZE) {
    double v = lp[tid];
    for (int l = 1; l < EPST_ENVS; ++l) v = EpstSlots::combine(tid, v, lp[l * KBJ_EPST_SIZE + tid]);
    part_out[(size_t)blockIdx.x * KBJ_EPST_SIZE + tid] = v;
  }
}

}  // namespace
}  // namespace kbj
