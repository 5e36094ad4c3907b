// kbj_push_recovery.h — what became of one scheduled push per env (kbj_push_recovery): from the per-row tracking errors kbj_tracking_stats
// left in err_d and the DONE column of the aux rows, the outcome of the push, the rows to recovery or to the fall and the peak errors on the
// way (KBJ_POUT_*, KBJ_PREC_*), then per group of envs their ordered statistics (KBJ_PSTAT_*). Included by kbj_traj_stats.hip.
//
// The rule. "Within" on row t: err[t][k] <= tol[k] for every error k whose tolerance is not +inf (a NaN error is not within; a column whose
// tolerance is +inf is not looked at, whatever it holds - a NaN too).
// An env's schedule is (s, d): the push is applied during the d rows s .. s + d - 1 (d < 0 counts as 0). With hold = hold_steps and
// window = window_steps:
//   s < 0: NONE.
//   VOID: s >= T, or s < hold, or any of the rows [s - hold, s) is not within or has DONE != 0.
//   Otherwise the rows t = s .. min(T, s + d + window) - 1 are scanned in order. On each row first the peaks: PEAK_LIN, PEAK_YAW, PEAK_TILT
//   and PEAK_HEIGHT become the row's error where it is greater (they start at -1; a NaN is never greater), and PEAK_ROW = t whenever
//   PEAK_TILT rises. Then, in this order:
//     1. DONE[t] < 0: FELL, FALL_STEPS = t - s. Stop.
//     2. DONE[t] > 0: CENSORED. Stop.
//     3. for t >= s + d the length of the run of consecutive within rows is kept (a row that is not within returns it to 0); when it
//        reaches hold: RECOVERED, RECOVER_STEPS = (t - hold + 1) - (s + d). Stop.
//   Undecided at the end: CENSORED if s + d + window > T (the trajectory cut the window), else UNRECOVERED.
//   Fields that do not apply are -1 (every field but the outcome for NONE and VOID).
//
// Shape. window_walk (kbj_window_scan.h) over chunks of PR_TC rows. For a fixed t the workgroup's err_d rows are 2 KB of contiguous floats,
// 32 bytes per lane: a lane fetches its own row (one 16-byte load, one 4-byte load for the fifth error) and its DONE word from the aux row.
// The common early end of the walk: an untrained policy's pushes are VOID on the hold rows. No LDS, no atomics.
// Second stage (when stats are asked for): push_recovery_reduce_kernel, the group reduce of kbj_window_scan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "kbj.h"
#include "kbj_window_scan.h"

namespace kbj {
namespace {

constexpr int PR_TC = 8;             // rows per chunk: 6 registers a row, two images
static_assert(KBJ_TERR_SIZE == 8 && KBJ_NTERR == 5 && KBJ_TERR_LIN == 0 && KBJ_TERR_HEIGHT == 3 && KBJ_TERR_ARM == 4, "an err_d row: four peak errors in the first 16 bytes, the fifth error behind them");
static_assert(KBJ_PREC_SIZE == 8 && KBJ_PREC_PEAK_LIN + KBJ_NPEAK == KBJ_PREC_PEAK_ROW && KBJ_PSTAT_PEAK_MAX + KBJ_NPEAK <= KBJ_PSTAT_SIZE, "push recovery layout");
static_assert(KBJ_POUT_COUNT == KBJ_PSTAT_REC_SUM - KBJ_PSTAT_COUNT, "one count per outcome");

struct PrRow { float4 e; float arm, done; };
// one error against its tolerance: +inf switches the column off (its NaN passes too), otherwise a NaN fails
__device__ inline bool pr_within(float e, float tol) { return tol == INFINITY || e <= tol; }

// grid = ceil(N / 64) workgroups of one wavefront; err [T][N][KBJ_TERR_SIZE], aux [T + 1][N][KBJ_AUX_SIZE], sched [N][2], rec [N][KBJ_PREC_SIZE]
__global__ __launch_bounds__(WINDOW_ENVS) void push_recovery_kernel(const float* __restrict__ err, const float* __restrict__ aux, int T, int N, const int32_t* __restrict__ sched,
                                                                     kbj_push_criteria crit, float* __restrict__ rec) {
  const int lane = threadIdx.x, env = blockIdx.x * WINDOW_ENVS + lane;
  const bool live = env < N;
  const int hold = crit.hold_steps;
  int s = -1, d = 0;
  if (live) { const int2 sd = reinterpret_cast<const int2*>(sched)[env]; s = sd.x; d = max(sd.y, 0); }
  const Window w(live, s, hold, (long long)d + crit.window_steps, T);     // hold >= 1: a scanned s is >= 0 too
  const long long post64 = (long long)s + d;
  const int post = post64 < (long long)INT_MAX ? (int)post64 : INT_MAX;              // first row behind the push

  int outcome = !live || s < 0 ? KBJ_POUT_NONE : KBJ_POUT_VOID;     // a scanned env: VOID until its pre-push rows have passed
  bool decided = !w.scan;
  int run = 0;
  float peak[KBJ_NPEAK] = {-1.0f, -1.0f, -1.0f, -1.0f}, peak_row = -1.0f, rec_steps = -1.0f, fall_steps = -1.0f;

  window_walk<PR_TC, PrRow>(w, decided,
    [&](PrRow& r, int t) {
      const size_t i = (size_t)t * N + env;
      r.e = *reinterpret_cast<const float4*>(err + i * KBJ_TERR_SIZE);
      r.arm = err[i * KBJ_TERR_SIZE + KBJ_TERR_ARM];
      r.done = aux[i * KBJ_AUX_SIZE + KBJ_AUX_DONE];
    },
    [&](const PrRow& r, int t) {
      const float e[KBJ_NPEAK] = {r.e.x, r.e.y, r.e.z, r.e.w};
      const float done = r.done;
      const bool within = pr_within(e[0], crit.tol[0]) && pr_within(e[1], crit.tol[1]) && pr_within(e[2], crit.tol[2]) && pr_within(e[3], crit.tol[3]) &&
                          pr_within(r.arm, crit.tol[4]);
      if (t < s) {                                            // the hold rows in front of the push
        if (!within || done != 0.0f) decided = true;          // stays VOID
        return;
      }
      if (e[KBJ_TERR_TILT] > peak[KBJ_TERR_TILT]) peak_row = (float)t;
#pragma unroll
      for (int j = 0; j < KBJ_NPEAK; ++j) if (e[j] > peak[j]) peak[j] = e[j];
      if (done < 0.0f) { outcome = KBJ_POUT_FELL; fall_steps = (float)(t - s); decided = true; }
      else if (done > 0.0f) { outcome = KBJ_POUT_CENSORED; decided = true; }
      else if (t >= post) {
        run = within ? run + 1 : 0;
        if (run >= hold) { outcome = KBJ_POUT_RECOVERED; rec_steps = (float)((t - hold + 1) - post); decided = true; }
      }
    });
  if (w.scan && !decided) outcome = w.end64 > (long long)T ? KBJ_POUT_CENSORED : KBJ_POUT_UNRECOVERED;    // the hold rows passed, the window ran out
  if (live) {
    float4* o = reinterpret_cast<float4*>(rec + (size_t)env * KBJ_PREC_SIZE);
    o[0] = make_float4((float)outcome, rec_steps, fall_steps, peak[0]);
    o[1] = make_float4(peak[1], peak[2], peak[3], peak_row);
  }
}

// one workgroup of GROUP_REDUCE_THREADS; thread g < G: group g's statistics over the envs in env order -> stats [G][KBJ_PSTAT_SIZE]. group == null: every
// env is in group 0; an env whose group is outside [0, G) is in none.
__global__ __launch_bounds__(GROUP_REDUCE_THREADS) void push_recovery_reduce_kernel(const float* __restrict__ rec, const int32_t* __restrict__ group, int N, int G,
                                                                               double* __restrict__ stats) {
  __shared__ __align__(16) float row[GROUP_REDUCE_THREADS][KBJ_PREC_SIZE];
  __shared__ int grp[GROUP_REDUCE_THREADS];
  const int g = threadIdx.x;
  int cnt[KBJ_POUT_COUNT] = {0, 0, 0, 0, 0, 0};
  double rs = 0, rq = 0, rm = -1, fs = 0, fq = 0, fm = -1, ps[KBJ_NPEAK] = {0, 0, 0, 0}, pm[KBJ_NPEAK] = {-1, -1, -1, -1};
  for (int n0 = 0; n0 < N; n0 += GROUP_REDUCE_THREADS) {
    const int nb = min(GROUP_REDUCE_THREADS, N - n0);
    group_stage_round(row, grp, rec, group, n0, nb);
    if (g < G) {
      for (int i = 0; i < nb; ++i) {
        if (grp[i] != g) continue;
        const float4 r0 = reinterpret_cast<const float4*>(row[i])[0], r1 = reinterpret_cast<const float4*>(row[i])[1];
        const int oc = (int)r0.x;
#pragma unroll
        for (int k = 0; k < KBJ_POUT_COUNT; ++k) cnt[k] += oc == k;
        if (oc == KBJ_POUT_RECOVERED) { const double x = (double)r0.y; rs += x; rq += x * x; rm = fmax(rm, x); }
        if (oc == KBJ_POUT_FELL) { const double x = (double)r0.z; fs += x; fq += x * x; fm = fmax(fm, x); }
        if (oc >= KBJ_POUT_FELL) {
          const double p[KBJ_NPEAK] = {(double)r0.w, (double)r1.x, (double)r1.y, (double)r1.z};
#pragma unroll
          for (int j = 0; j < KBJ_NPEAK; ++j) { ps[j] += p[j]; pm[j] = fmax(pm[j], p[j]); }
        }
      }
    }
  }
  if (g < G) {
    double* o = stats + (size_t)g * KBJ_PSTAT_SIZE;
#pragma unroll
    for (int k = 0; k < KBJ_POUT_COUNT; ++k) o[KBJ_PSTAT_COUNT + k] = (double)cnt[k];
    o[KBJ_PSTAT_REC_SUM] = rs; o[KBJ_PSTAT_REC_SUMSQ] = rq; o[KBJ_PSTAT_REC_MAX] = rm;
    o[KBJ_PSTAT_FALL_SUM] = fs; o[KBJ_PSTAT_FALL_SUMSQ] = fq; o[KBJ_PSTAT_FALL_MAX] = fm;
#pragma unroll
    for (int j = 0; j < KBJ_NPEAK; ++j) { o[KBJ_PSTAT_PEAK_SUM + j] = ps[j]; o[KBJ_PSTAT_PEAK_MAX + j] = pm[j]; }
    for (int k = KBJ_PSTAT_PEAK_MAX + KBJ_NPEAK; k < KBJ_PSTAT_SIZE; ++k) o[k] = 0.0;
  }
}

}  // namespace
}  // namespace kbj
