// kbj_robustness.h — whether a policy stays up and on its command over a whole trajectory (kbj_robustness): from the per-row tracking errors
// kbj_tracking_stats left in err_d and the DONE column of the aux rows, per env the falls, the time-outs, the first fall and the sums and
// maxima of the five errors over the settled rows (KBJ_RREC_*), then per group of envs their ordered statistics (KBJ_RSTAT_*). The rule is in
// include/kbj.h at kbj_robustness, word for word; tests/robustness_ref.py restates it; survival, falls per second and the mean errors are
// host arithmetic on the slots (host/robustness.py). Included by kbj_traj_stats.hip.
//
// Shapes.
// robustness_scan_kernel: window_walk (kbj_window_scan.h) over chunks of RB_TC rows; the window of every lane is the whole trajectory
// (s = 0, no hold rows, a tail of T rows), so no lane is ever decided and the walk ends with the last chunk. For a fixed t the workgroup's
// err_d rows are 2 KB of contiguous floats: a lane fetches its row as two 16-byte loads and its DONE word from the aux row - 36 bytes per
// (row, env). The accumulators are locals: 4 counters, 10 double sums, 5 fp32 maxima. No LDS, no atomics.
// Second stage (when stats are asked for): robustness_reduce_kernel, the group reduce of kbj_window_scan.h on records of 24 doubles staged as
// 48 floats.
#pragma once
#include <hip/hip_runtime.h>
#include "kbj.h"
#include "kbj_window_scan.h"

namespace kbj {
namespace {

constexpr int RB_TC = 4;          // rows per chunk: 9 registers a row, two images
constexpr int RB_REC_FLOATS = 2 * KBJ_RREC_SIZE;   // a record of doubles as the group reduce stages it
static_assert(KBJ_TERR_SIZE == 8 && KBJ_NTERR == 5 && KBJ_TERR_LIN == 0 && KBJ_TERR_ARM == 4 && KBJ_TERR_SETTLED == 6, "an err_d row: four errors in the first 16 bytes, the fifth and the settled flag in the second");
static_assert(KBJ_RREC_ERR_SUM + KBJ_NTERR == KBJ_RREC_ERR_SUMSQ && KBJ_RREC_ERR_SUMSQ + KBJ_NTERR == KBJ_RREC_ERR_MAX && KBJ_RREC_ERR_MAX + KBJ_NTERR <= KBJ_RREC_SIZE, "robustness record layout");
static_assert(KBJ_RREC_SIZE % 2 == 0 && RB_REC_FLOATS % 4 == 0, "a record is written and staged as 16-byte pieces");
static_assert(KBJ_RSTAT_ERR_SUM + KBJ_NTERR == KBJ_RSTAT_ERR_SUMSQ && KBJ_RSTAT_ERR_SUMSQ + KBJ_NTERR == KBJ_RSTAT_ERR_MAX && KBJ_RSTAT_ERR_MAX + KBJ_NTERR <= KBJ_RSTAT_SIZE, "robustness statistics layout");

struct RbRow { float4 e, f; float done; };     // e: the first four errors; f: ARM, MODE, SETTLED, SINCE

// grid = ceil(N / 64) workgroups of one wavefront; err [T][N][KBJ_TERR_SIZE], aux [T + 1][N][KBJ_AUX_SIZE], rec [N][KBJ_RREC_SIZE] doubles (16-byte aligned)
__global__ __launch_bounds__(WINDOW_ENVS) void robustness_scan_kernel(const float* __restrict__ err, const float* __restrict__ aux, int T, int N, double* __restrict__ rec) {
  const int lane = threadIdx.x, env = blockIdx.x * WINDOW_ENVS + lane;
  const bool live = env < N;
  const Window w(live, 0, 0, (long long)T, T);                 // the whole trajectory: rows [0, T)
  bool decided = !w.scan;                                      // a live lane never is: every row counts

  int rows = 0, falls = 0, timeouts = 0, first_fall = -1, settled = 0;
  double sum[KBJ_NTERR] = {0.0, 0.0, 0.0, 0.0, 0.0}, sumsq[KBJ_NTERR] = {0.0, 0.0, 0.0, 0.0, 0.0};
  float emax[KBJ_NTERR] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f};

  window_walk<RB_TC, RbRow>(w, decided,
    [&](RbRow& r, int t) {
      const size_t i = (size_t)t * N + env;
      const float4* p = reinterpret_cast<const float4*>(err + i * KBJ_TERR_SIZE);
      r.e = p[0]; r.f = p[1];
      r.done = aux[i * KBJ_AUX_SIZE + KBJ_AUX_DONE];
    },
    [&](const RbRow& r, int t) {
      const float done = r.done;
      rows += 1;
      if (done < 0.0f) { falls += 1; if (first_fall < 0) first_fall = t; }
      if (done > 0.0f) timeouts += 1;
      if (r.f.z != 0.0f) {                                      // KBJ_TERR_SETTLED
        settled += 1;
        const float e[KBJ_NTERR] = {r.e.x, r.e.y, r.e.z, r.e.w, r.f.x};
#pragma unroll
        for (int k = 0; k < KBJ_NTERR; ++k) {
          const double x = (double)e[k];
          sum[k] += x; sumsq[k] += x * x;
          if (e[k] > emax[k]) emax[k] = e[k];
        }
      }
    });
  if (live) {
    double2* o = reinterpret_cast<double2*>(rec + (size_t)env * KBJ_RREC_SIZE);
    double v[KBJ_RREC_SIZE];
#pragma unroll
    for (int k = 0; k < KBJ_RREC_SIZE; ++k) v[k] = 0.0;
    v[KBJ_RREC_ROWS] = (double)rows; v[KBJ_RREC_FALLS] = (double)falls; v[KBJ_RREC_TIMEOUTS] = (double)timeouts;
    v[KBJ_RREC_FIRST_FALL] = (double)first_fall; v[KBJ_RREC_SETTLED] = (double)settled;
#pragma unroll
    for (int k = 0; k < KBJ_NTERR; ++k) { v[KBJ_RREC_ERR_SUM + k] = sum[k]; v[KBJ_RREC_ERR_SUMSQ + k] = sumsq[k]; v[KBJ_RREC_ERR_MAX + k] = (double)emax[k]; }
#pragma unroll
    for (int k = 0; k < KBJ_RREC_SIZE / 2; ++k) o[k] = make_double2(v[2 * k], v[2 * k + 1]);
  }
}

// one workgroup of GROUP_REDUCE_THREADS; thread g < G: group g's statistics over the envs in env order -> stats [G][KBJ_RSTAT_SIZE]. group == null: every
// env is in group 0; an env whose group is outside [0, G) is in none. rec [N][KBJ_RREC_SIZE] doubles (16-byte aligned), staged as RB_REC_FLOATS floats a record.
__global__ __launch_bounds__(GROUP_REDUCE_THREADS) void robustness_reduce_kernel(const double* __restrict__ rec, const int32_t* __restrict__ group, int N, int G,
                                                                                 double* __restrict__ stats) {
  __shared__ __align__(16) float row[GROUP_REDUCE_THREADS][RB_REC_FLOATS];
  __shared__ int grp[GROUP_REDUCE_THREADS];
  const int g = threadIdx.x;
  int envs = 0, fell = 0;
  double falls = 0.0, timeouts = 0.0, rows = 0.0, settled = 0.0, ff_sum = 0.0, ff_min = -1.0;
  double sum[KBJ_NTERR] = {0.0, 0.0, 0.0, 0.0, 0.0}, sumsq[KBJ_NTERR] = {0.0, 0.0, 0.0, 0.0, 0.0}, emax[KBJ_NTERR] = {-1.0, -1.0, -1.0, -1.0, -1.0};
  for (int n0 = 0; n0 < N; n0 += GROUP_REDUCE_THREADS) {
    const int nb = min(GROUP_REDUCE_THREADS, N - n0);
    group_stage_round(row, grp, reinterpret_cast<const float*>(rec), group, n0, nb);
    if (g < G) {
      for (int i = 0; i < nb; ++i) {
        if (grp[i] != g) continue;
        const double* r = reinterpret_cast<const double*>(row[i]);
        envs += 1;
        falls += r[KBJ_RREC_FALLS]; timeouts += r[KBJ_RREC_TIMEOUTS]; rows += r[KBJ_RREC_ROWS]; settled += r[KBJ_RREC_SETTLED];
        const double ff = r[KBJ_RREC_FIRST_FALL];
        if (ff >= 0.0) { fell += 1; ff_sum += ff; ff_min = (ff_min < 0.0 || ff < ff_min) ? ff : ff_min; }
#pragma unroll
        for (int k = 0; k < KBJ_NTERR; ++k) {
          sum[k] += r[KBJ_RREC_ERR_SUM + k]; sumsq[k] += r[KBJ_RREC_ERR_SUMSQ + k];
          const double x = r[KBJ_RREC_ERR_MAX + k];
          emax[k] = x > emax[k] ? x : emax[k];
        }
      }
    }
  }
  if (g < G) {
    double* o = stats + (size_t)g * KBJ_RSTAT_SIZE;
    o[KBJ_RSTAT_ENVS] = (double)envs; o[KBJ_RSTAT_FELL_ENVS] = (double)fell; o[KBJ_RSTAT_FALLS] = falls; o[KBJ_RSTAT_TIMEOUTS] = timeouts;
    o[KBJ_RSTAT_ROWS] = rows; o[KBJ_RSTAT_FIRST_FALL_SUM] = ff_sum; o[KBJ_RSTAT_FIRST_FALL_MIN] = ff_min; o[KBJ_RSTAT_SETTLED] = settled;
#pragma unroll
    for (int k = 0; k < KBJ_NTERR; ++k) { o[KBJ_RSTAT_ERR_SUM + k] = sum[k]; o[KBJ_RSTAT_ERR_SUMSQ + k] = sumsq[k]; o[KBJ_RSTAT_ERR_MAX + k] = emax[k]; }
    for (int k = KBJ_RSTAT_ERR_MAX + KBJ_NTERR; k < KBJ_RSTAT_SIZE; ++k) o[k] = 0.0;
  }
}

}  // namespace
}  // namespace kbj
