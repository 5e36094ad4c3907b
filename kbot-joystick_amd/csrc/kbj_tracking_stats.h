// kbj_tracking_stats.h — command-tracking errors over one trajectory (kbj_tracking_stats): the five tracking errors of every aux row in
// physical units, split by the command mode of the row, counted over the rows whose command has been held for settle_steps rows
// (KBJ_TACC_*, KBJ_TRK_*, KBJ_TERR_*, KBJ_CMODE_*). Included by kbj_traj_stats.hip, behind kbj_env_core.h (quat_to_euler & co).
//
// Shape: episode_stats_kernel's. One workgroup of seven wavefronts owns 64 consecutive envs. For a fixed t the block's aux rows are 18 KB of
// contiguous floats: wavefronts 1-6 each fetch one time step of a 6-step chunk with 18 coalesced 16-byte loads per lane (issued one chunk
// ahead, so they fly under the evaluation of the chunk before), stage the 12 pieces the errors read (kbj_aux_stage.h: a row stride of 49
// words) and evaluate the five errors there, one env per lane: the rows are independent, so the
// trigonometry runs on the wide part, two wavefronts per SIMD. What is left per row - five errors, the mode, DONE, "same command as the
// row before" - is six words. Wavefront 0 runs the ordered part from them, one env per lane: rows since the command changed or the episode
// started, the settled test, the per-mode sums.
// The per-mode accumulators are indexed by a run-time mode, so they do not live in registers (they would become scratch): they are an LDS
// image [mode][slot][lane] of doubles (52 KB; the lane is the fastest index: conflict-free). Lanes are combined in lane order, the
// workgroup partials in block order by a second, single-workgroup kernel (kbj_ordered_reduce.h over TrkSlots): doubles, fixed order, no atomics - a call is bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "kbj_model.h"
#include "kbj_aux_stage.h"
#include "kbj_ordered_reduce.h"

namespace kbj {
namespace {

constexpr int TRK_ENVS = 64;        // envs per workgroup = lanes of every wavefront
constexpr int TRK_THREADS = 448;    // wavefront 0 scans, wavefronts 1-6 stage and evaluate
constexpr int TRK_TC = 6;           // time steps per chunk: one per staging wavefront
constexpr int TRK_V4 = AUX_V4;      // loads per lane and time step: every 16-byte piece of an aux row
constexpr int TRK_RES = KBJ_NTERR + 1;               // words per evaluated row: the errors and the flags word
constexpr int TRK_SLOTS = KBJ_TRK_MAX + KBJ_NTERR;   // used slots of a mode block
constexpr int TRK_IMG = KBJ_CMODE_COUNT * TRK_SLOTS + 2;   // rows of the accumulator image: the mode blocks, command changes, episodes started
static_assert(KBJ_AUX_SIZE % 4 == 0 && KBJ_TACC_SIZE % 4 == 0 && KBJ_TACC_SINCE == KBJ_NCMD && KBJ_TACC_RUNNING == KBJ_TACC_SINCE + 1, "tracking layout: 16-byte pieces");
static_assert(KBJ_TRK_SUM == 2 && KBJ_TRK_SUMSQ == KBJ_TRK_SUM + KBJ_NTERR && KBJ_TRK_MAX == KBJ_TRK_SUMSQ + KBJ_NTERR && TRK_SLOTS <= KBJ_TRK_MODE_STRIDE &&
              KBJ_CMODE_COUNT * KBJ_TRK_MODE_STRIDE == KBJ_TRK_CHANGES && KBJ_TRK_EPISODES < KBJ_TRK_SIZE && KBJ_TRK_SIZE <= TRK_THREADS, "tracking statistics layout");
static_assert(TRK_THREADS == 64 * (TRK_TC + 1), "one scanning wavefront and one staging wavefront per time step of a chunk");

// the staged pieces of an aux row (kbj_aux_stage.h): those the errors read are 0-3 (QVEL, BQUAT, BASEZ, LFZ, RFZ), 5-7 (ARMQ) and 13-17
// (CMD, DONE)
struct TrkMap {
  static constexpr int NPIECE = 12;
  static __device__ constexpr int piece(int p) { return p < 4 ? p : (p >= 5 && p <= 7) ? p - 1 : (p >= 13 && p <= 17) ? p - 6 : -1; }
};
using TrkRow = StagedRow<TrkMap>;
constexpr int TRK_LD = TrkRow::LD;
static_assert(TrkMap::piece(KBJ_AUX_RFZ / 4) == 3 && TrkMap::piece(4) == -1 && TrkMap::piece(KBJ_AUX_ARMQ / 4) == 4 && TrkMap::piece((KBJ_AUX_ARMQ + 9) / 4) == 6 &&
              TrkMap::piece(8) == -1 && TrkMap::piece(12) == -1 && TrkMap::piece(KBJ_AUX_CMD / 4) == 7 && TrkMap::piece(KBJ_AUX_DONE / 4) == 11 && TRK_LD == 49 &&
              KBJ_AUX_SIZE / 4 == 18, "staged pieces");

struct TrkShared {
  double img[TRK_IMG][TRK_ENVS];                 // [mode * TRK_SLOTS + slot][lane], then changes, episodes
  float raw[TRK_TC][TRK_ENVS * TRK_LD];          // the chunk's aux rows, [tt][env * TRK_LD + column]
  float res[2][TRK_TC][TRK_RES][TRK_ENVS];       // evaluated rows of chunk c in res[c & 1]: [tt][error | flags][env]
  float last[2][KBJ_NCMD][TRK_ENVS];             // the command of the last row of chunk c in last[c & 1]
};

// the slots of a KBJ_TRK vector (kbj_ordered_reduce.h): counts and sums, but for the maxima of each mode block (the errors are non-negative)
struct TrkSlots : SumMaxSlots<TrkSlots> {
  static constexpr int SIZE = KBJ_TRK_SIZE;
  static __device__ inline bool is_max(int j) { return j < KBJ_TRK_CHANGES && j % KBJ_TRK_MODE_STRIDE >= KBJ_TRK_MAX && j % KBJ_TRK_MODE_STRIDE < KBJ_TRK_MAX + KBJ_NTERR; }
};

// the five errors of one staged aux row: rewards_kernel's expressions (kbj_traj_stats.hip), before their exp. Restated, not shared: called
// from one template over the row type, rewards_kernel contracts its multiply-adds differently (other fma / packed-fma counts), so reward
// bits could move. tests/test_gpu_tracking_stats.py test_reward_terms_follow_from_the_error_rows ties the two restatements together
__device__ inline void trk_errors(const TrkRow a, const float* __restrict__ joint_bias, float standard_height, float foot_origin_height, float* e) {
  float cmd[KBJ_NCMD];
#pragma unroll
  for (int k = 0; k < KBJ_NCMD; ++k) cmd[k] = a[KBJ_AUX_CMD + k];
  float bq[4] = {a[KBJ_AUX_BQUAT], a[KBJ_AUX_BQUAT + 1], a[KBJ_AUX_BQUAT + 2], a[KBJ_AUX_BQUAT + 3]}, be[3];
  quat_to_euler(bq, be);
  {
    float ye[3] = {0, 0, be[2]}, yq[4], v[3] = {cmd[0], cmd[1], 0}, g[3];
    euler_to_quat(ye, yq); rotate_by_quat(v, yq, false, g);
    float ex = a[KBJ_AUX_QVEL] - g[0], ey = a[KBJ_AUX_QVEL + 1] - g[1];
    e[KBJ_TERR_LIN] = sqrtf(ex * ex + ey * ey);
  }
  e[KBJ_TERR_YAW] = fabsf(a[KBJ_AUX_QVEL + 5] - cmd[2]);
  {
    float e1[3] = {be[0], be[1], 0}, q1[4], e2[3] = {cmd[4], cmd[5], 0}, q2[4];
    euler_to_quat(e1, q1); euler_to_quat(e2, q2);
    float d_ = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3];
    e[KBJ_TERR_TILT] = 1 - d_ * d_;
  }
  {
    float low = fminf(a[KBJ_AUX_LFZ] - foot_origin_height, a[KBJ_AUX_RFZ] - foot_origin_height);
    float h = a[KBJ_AUX_BASEZ] - low;
    e[KBJ_TERR_HEIGHT] = fabsf(h - (cmd[3] + standard_height));
  }
  {
    float s = 0;
#pragma unroll
    for (int j = 0; j < 10; ++j) { float dq = a[KBJ_AUX_ARMQ + j] - (cmd[6 + j] + joint_bias[10 + j]); s += dq * dq; }
    e[KBJ_TERR_ARM] = s;
  }
}

// grid = ceil(N / 64) workgroups of 448 threads; part_out [gridDim.x][KBJ_TRK_SIZE]; err [T][N][KBJ_TERR_SIZE] or null
__global__ __launch_bounds__(TRK_THREADS) void tracking_stats_kernel(const kbj_model* __restrict__ m, const float* __restrict__ aux, int T, int N, int settle_steps,
                                                                      float standard_height, float foot_origin_height, float* __restrict__ acc,
                                                                      double* __restrict__ part_out, float* __restrict__ err) {
  __shared__ __align__(16) TrkShared S;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int e0 = blockIdx.x * TRK_ENVS, nb = min(TRK_ENVS, N - e0);
  const int nchunk = (T + TRK_TC - 1) / TRK_TC;
  const int npiece = nb * TRK_V4;                 // 16-byte pieces of the block's rows of one time step
  const bool live = lane < nb;
  float* row = acc + (size_t)(e0 + lane) * KBJ_TACC_SIZE;

  for (int i = tid; i < TRK_IMG * TRK_ENVS; i += TRK_THREADS) (&S.img[0][0])[i] = 0.0;

  // scanner state (wavefront 0) and the carried command (wavefront 1, for row 0): read before anybody writes the row back. The wavefront that
  // owns row T - 1 overwrites these 64 bytes, possibly in chunk 0 already (T <= TRK_TC): the loop's first __syncthreads, between this load and
  // any such store, is what orders the two - nothing else does
  float since = 0, running = 0, prev[KBJ_NCMD];
  int n_changes = 0, n_episodes = 0;
  if (live && wave == 0) { since = row[KBJ_TACC_SINCE]; running = row[KBJ_TACC_RUNNING]; }
  if (live && wave == 1) {
#pragma unroll
    for (int q = 0; q < KBJ_NCMD / 4; ++q) {
      const float4 p = reinterpret_cast<const float4*>(row)[q];
      prev[4 * q] = p.x; prev[4 * q + 1] = p.y; prev[4 * q + 2] = p.z; prev[4 * q + 3] = p.w;
    }
  }

  // staging registers: the pieces lane, lane + 64, ... of time step t0 + wave - 1
  float4 v[TRK_V4];
  auto fetch = [&](int c, int k0, int k1) {
    const int t = c * TRK_TC + wave - 1;
    if (wave == 0 || t >= T) return;
    const float4* src = reinterpret_cast<const float4*>(aux + ((size_t)t * N + e0) * KBJ_AUX_SIZE);
#pragma unroll
    for (int k = 0; k < TRK_V4; ++k)
      if (k >= k0 && k < k1 && k * 64 + lane < npiece) v[k] = src[k * 64 + lane];
  };
  fetch(0, 0, TRK_V4);

  for (int c = 0; c <= nchunk; ++c) {
    const int tt = wave - 1, t = c * TRK_TC + tt;
    const bool mine = wave > 0 && c < nchunk && t < T;     // this wavefront has a time step in chunk c
    if (mine) {
#pragma unroll
      for (int k = 0; k < TRK_V4; ++k) stage_piece<TrkMap>(S.raw[tt], v[k], k * 64 + lane, npiece);
    }
    __syncthreads();
    if (wave > 0) {
      if (c + 1 < nchunk) fetch(c + 1, 0, TRK_V4 / 2);      // half of the next chunk's loads fly under the evaluation, the other half (registers) behind it
      if (mine && live) {
        const TrkRow a{S.raw[tt] + lane * TRK_LD};
        float cmd[KBJ_NCMD];
#pragma unroll
        for (int k = 0; k < KBJ_NCMD; ++k) cmd[k] = a[KBJ_AUX_CMD + k];
        float e[KBJ_NTERR];
        trk_errors(a, m->joint_bias, standard_height, foot_origin_height, e);
        bool same = true;
        if (tt > 0) {
          const TrkRow p{S.raw[tt - 1] + lane * TRK_LD};
#pragma unroll
          for (int k = 0; k < KBJ_NCMD; ++k) same = same && !(cmd[k] != p[KBJ_AUX_CMD + k]);
        } else if (c > 0) {
#pragma unroll
          for (int k = 0; k < KBJ_NCMD; ++k) same = same && !(cmd[k] != S.last[(c - 1) & 1][k][lane]);
        } else {
#pragma unroll
          for (int k = 0; k < KBJ_NCMD; ++k) same = same && !(cmd[k] != prev[k]);
        }
        const int flags = cmd_mode(a) | (same ? 8 : 0) | (a[KBJ_AUX_DONE] != 0.0f ? 16 : 0);
        float (*r)[TRK_ENVS] = S.res[c & 1][tt];
#pragma unroll
        for (int k = 0; k < KBJ_NTERR; ++k) r[k][lane] = e[k];
        r[KBJ_NTERR][lane] = __int_as_float(flags);
        if (tt == TRK_TC - 1) {
#pragma unroll
          for (int k = 0; k < KBJ_NCMD; ++k) S.last[c & 1][k][lane] = cmd[k];
        }
        if (t == T - 1) {        // the env's last row: its command is what the next call compares row 0 with
#pragma unroll
          for (int q = 0; q < KBJ_NCMD / 4; ++q) reinterpret_cast<float4*>(row)[q] = make_float4(cmd[4 * q], cmd[4 * q + 1], cmd[4 * q + 2], cmd[4 * q + 3]);
        }
      }
      if (c + 1 < nchunk) fetch(c + 1, TRK_V4 / 2, TRK_V4);
    } else if (live && c > 0) {      // ordered scan of chunk c - 1
      const int t0 = (c - 1) * TRK_TC, tc = min(TRK_TC, T - t0);
      for (int s = 0; s < tc; ++s) {
        const float (*r)[TRK_ENVS] = S.res[(c - 1) & 1][s];
        const int flags = __float_as_int(r[KBJ_NTERR][lane]), mode = flags & 7;
        const bool same = flags & 8, run = running != 0.0f;
        n_episodes += !run; n_changes += run && !same;
        since = (run && same) ? fminf(since + 1.0f, 16777216.0f) : 0.0f;
        const bool settled = (int)since >= settle_steps;
        running = (flags & 16) ? 0.0f : 1.0f;
        double (*A)[TRK_ENVS] = S.img + mode * TRK_SLOTS;
        A[KBJ_TRK_ROWS][lane] += 1.0;
        float e[KBJ_NTERR];
#pragma unroll
        for (int k = 0; k < KBJ_NTERR; ++k) e[k] = r[k][lane];
        if (settled) {
          A[KBJ_TRK_SETTLED][lane] += 1.0;
#pragma unroll
          for (int k = 0; k < KBJ_NTERR; ++k) {
            const double x = (double)e[k];
            A[KBJ_TRK_SUM + k][lane] += x;
            A[KBJ_TRK_SUMSQ + k][lane] += x * x;
            A[KBJ_TRK_MAX + k][lane] = fmax(A[KBJ_TRK_MAX + k][lane], x);
          }
        }
        if (err) {
          float4* o = reinterpret_cast<float4*>(err + ((size_t)(t0 + s) * N + e0 + lane) * KBJ_TERR_SIZE);
          o[0] = make_float4(e[0], e[1], e[2], e[3]);
          o[1] = make_float4(e[4], (float)mode, settled ? 1.0f : 0.0f, since);
        }
      }
    }
    __syncthreads();
  }

  if (wave == 0) {
    if (live) *reinterpret_cast<float2*>(row + KBJ_TACC_SINCE) = make_float2(since, running);
    S.img[TRK_IMG - 2][lane] = (double)n_changes; S.img[TRK_IMG - 1][lane] = (double)n_episodes;     // lanes beyond the last env hold 0
  }
  __syncthreads();
  if (tid < KBJ_TRK_SIZE) {        // slot tid of the partial: the lanes in lane order
    const int mode = tid / KBJ_TRK_MODE_STRIDE, slot = tid % KBJ_TRK_MODE_STRIDE;
    const int r = tid < KBJ_TRK_CHANGES ? (slot < TRK_SLOTS ? mode * TRK_SLOTS + slot : -1) : tid <= KBJ_TRK_EPISODES ? TRK_IMG - 2 + (tid - KBJ_TRK_CHANGES) : -1;
    double x = 0.0;
    if (r >= 0) {
      const bool is_max = TrkSlots::is_max(tid);
      x = S.img[r][0];
      for (int l = 1; l < TRK_ENVS; ++l) x = TrkSlots::combine_as(is_max, x, S.img[r][l]);
    }
    part_out[(size_t)blockIdx.x * KBJ_TRK_SIZE + tid] = x;
  }
}

}  // namespace
}  // namespace kbj
