// kbj_step_response.h — what the robot does when the stick moves (kbj_step_response): from the aux rows a response signal per row (KBJ_SSIG_*:
// base velocity in the heading frame, yaw rate, the three command words, DONE), then per env the outcome of ONE scheduled command change, its
// rise time, overshoot, settling time, travel and cross-coupling (KBJ_SOUT_*, KBJ_SREC_*), then per group of envs their ordered statistics
// (KBJ_SSTAT_*). The rule is in include/kbj.h at kbj_step_response, word for word; tests/step_response_ref.py restates it. Included by
// kbj_traj_stats.hip.
//
// Shapes.
// step_signal_kernel: elementwise over the T N rows, one thread per row. Of the 288 bytes of an aux row it fetches the first 40 (two 16-byte
// loads, one 8-byte load: QVEL and BQUAT), the three command words (KBJ_AUX_CMD is 8-byte aligned: one 8-byte and one 4-byte load) and DONE
// (4 bytes), and writes the 32-byte signal row as two float4 stores.
// step_scan_kernel: window_walk (kbj_window_scan.h) over chunks of SR_TC rows; for a fixed t the workgroup's signal rows are 2 KB of
// contiguous floats, 32 bytes per lane, fetched as two 16-byte loads. The trailing window of the smoothed value (up to 32 rows x 3 channels
// per lane) lives in an LDS ring [32][3][64] floats = 24 KB: slot (t & 31) of a row is uniform over the wavefront and the lane is the fastest
// index, so every access puts consecutive lanes on consecutive banks (no conflict) and no lane ever reads another lane's words (no barrier).
// The sum of S_k(t) is taken afresh on every row, ascending in u, in double: a running add / subtract would not be the same sum.
// Second stage (when stats are asked for): step_reduce_kernel, the group reduce of kbj_window_scan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "kbj.h"
#include "kbj_window_scan.h"

namespace kbj {
namespace {

constexpr int SR_TC = 4;              // rows per chunk: 8 registers a row, two images
constexpr int SR_RING = 32;           // rows of the smoothing ring = the largest smooth_steps
constexpr int SR_SIG_THREADS = 256;   // the signal kernel: one row per thread
static_assert(KBJ_AUX_SIZE % 4 == 0 && KBJ_AUX_QVEL == 0 && KBJ_AUX_BQUAT == 6 && KBJ_AUX_CMD % 2 == 0, "an aux row: QVEL and BQUAT in the first 40 bytes, CMD 8-byte aligned");
static_assert(KBJ_SSIG_SIZE == 8 && KBJ_SSIG_VX == 0 && KBJ_SSIG_DONE == 3 && KBJ_SSIG_CMD == 4 && KBJ_NSCH == 3, "a signal row: two float4");
static_assert(KBJ_SREC_SIZE == 20 && KBJ_SREC_RISE == 8 && KBJ_SREC_OVER == 11 && KBJ_SREC_DEV == 14 && KBJ_SREC_SPARE_TAIL == 17, "a record row: five float4");
static_assert(KBJ_SOUT_COUNT == KBJ_SSTAT_SETTLE_SUM - KBJ_SSTAT_COUNT && KBJ_SSTAT_TRAVEL_ABSMAX + KBJ_NSCH <= KBJ_SSTAT_SIZE, "step statistics layout");
static_assert((SR_RING & (SR_RING - 1)) == 0, "ring slots are taken with a mask");

// "replaced where the new value is greater": a NaN or a -0 never replaces the old value (kbj.h)
__device__ inline float sr_max(float old, float x) { return x > old ? x : old; }
__device__ inline double sr_max(double old, double x) { return x > old ? x : old; }

// grid-stride over the rows; aux [T][N][KBJ_AUX_SIZE] (16-byte aligned), sig [T][N][KBJ_SSIG_SIZE]
__global__ __launch_bounds__(SR_SIG_THREADS) void step_signal_kernel(const float* __restrict__ aux, size_t rows, float* __restrict__ sig) {
  for (size_t i = (size_t)blockIdx.x * SR_SIG_THREADS + threadIdx.x; i < rows; i += (size_t)gridDim.x * SR_SIG_THREADS) {
    const float* a = aux + i * KBJ_AUX_SIZE;
    const float4 q0 = reinterpret_cast<const float4*>(a)[0], q1 = reinterpret_cast<const float4*>(a)[1];   // qvel 0..3; qvel 4, 5, quat w, x
    const float2 q2 = *reinterpret_cast<const float2*>(a + 8);                                                // quat y, z
    const float2 c01 = *reinterpret_cast<const float2*>(a + KBJ_AUX_CMD);
    const float c2 = a[KBJ_AUX_CMD + 2], done = a[KBJ_AUX_DONE];
    const float w = q1.z, x = q1.w, y = q2.x, z = q2.y;
    const float sn = 2.0f * (w * z + x * y), cs = 1.0f - 2.0f * (y * y + z * z), h = sqrtf(sn * sn + cs * cs);
    const bool ok = h > 0.0f;
    const float c = ok ? cs / h : 1.0f, s = ok ? sn / h : 0.0f;
    float4* o = reinterpret_cast<float4*>(sig + i * KBJ_SSIG_SIZE);
    o[0] = make_float4(c * q0.x + s * q0.y, -s * q0.x + c * q0.y, q1.y, done);
    o[1] = make_float4(c01.x, c01.y, c2, 0.0f);
  }
}

struct SrRow { float4 v, c; };   // VX, VY, WZ, DONE; CMD[3], spare

// grid = ceil(N / 64) workgroups of one wavefront; sig [T][N][KBJ_SSIG_SIZE], sched [N], rec [N][KBJ_SREC_SIZE]
__global__ __launch_bounds__(WINDOW_ENVS) void step_scan_kernel(const float* __restrict__ sig, int T, int N, const int32_t* __restrict__ sched, kbj_step_criteria crit,
                                                                 float* __restrict__ rec) {
  __shared__ float ring[SR_RING][KBJ_NSCH][WINDOW_ENVS];
  const int lane = threadIdx.x, env = blockIdx.x * WINDOW_ENVS + lane;
  const bool live = env < N;
  const int m = crit.smooth_steps, hold = crit.hold_steps;
  const int s = live ? sched[env] : -1;
  const Window w(live, s, hold, (long long)crit.window_steps, T);     // hold >= 1: a scanned s is >= 1, rows s - 1 and s exist; window >= 1: end > s
  const int first = w.first;

  // the step itself: c0, c1 and what follows from them
  float c0[KBJ_NSCH] = {0, 0, 0}, c1[KBJ_NSCH] = {0, 0, 0}, band[KBJ_NSCH], thr[KBJ_NSCH];
  bool neg[KBJ_NSCH], act[KBJ_NSCH];
  if (w.scan) {
    const float4 a = *reinterpret_cast<const float4*>(sig + ((size_t)(s - 1) * N + env) * KBJ_SSIG_SIZE + KBJ_SSIG_CMD);
    const float4 b = *reinterpret_cast<const float4*>(sig + ((size_t)s * N + env) * KBJ_SSIG_SIZE + KBJ_SSIG_CMD);
    c0[0] = a.x; c0[1] = a.y; c0[2] = a.z; c1[0] = b.x; c1[1] = b.y; c1[2] = b.z;
  }
  int active = 0;
#pragma unroll
  for (int k = 0; k < KBJ_NSCH; ++k) {
    const float delta = __fsub_rn(c1[k], c0[k]), mag = fabsf(delta);
    neg[k] = !(delta > 0.0f);
    act[k] = mag >= crit.min_step[k];
    active |= act[k] ? 1 << k : 0;
    band[k] = sr_max(crit.band_abs[k], __fmul_rn(crit.band_frac, mag));
    thr[k] = __fmul_rn(crit.rise_level, mag);
  }

  int outcome = !live || s < 0 ? KBJ_SOUT_NONE : KBJ_SOUT_VOID;     // a scanned env: VOID until its rows in front of the step have passed
  bool decided = !w.scan || active == 0;
  int run = 0;
  float rise[KBJ_NSCH] = {-1.0f, -1.0f, -1.0f}, over[KBJ_NSCH] = {0.0f, 0.0f, 0.0f}, dev[KBJ_NSCH] = {0.0f, 0.0f, 0.0f};
  float settle_steps = -1.0f, fall_steps = -1.0f;
  double travel[KBJ_NSCH] = {0.0, 0.0, 0.0};

  window_walk<SR_TC, SrRow>(w, decided,
    [&](SrRow& r, int t) {
      const float4* p = reinterpret_cast<const float4*>(sig + ((size_t)t * N + env) * KBJ_SSIG_SIZE);
      r.v = p[0]; r.c = p[1];
    },
    [&](const SrRow& r, int t) {
      const float v[KBJ_NSCH] = {r.v.x, r.v.y, r.v.z}, cmd[KBJ_NSCH] = {r.c.x, r.c.y, r.c.z};
      const float done = r.v.w;
#pragma unroll
      for (int j = 0; j < KBJ_NSCH; ++j) ring[t & (SR_RING - 1)][j][lane] = v[j];
      if (t < s) {                                             // the hold rows in front of the step
        if (done != 0.0f || cmd[0] != c0[0] || cmd[1] != c0[1] || cmd[2] != c0[2]) { decided = true; return; }     // stays VOID
        if (t < s - 1) return;
      } else {
        if (done < 0.0f) { outcome = KBJ_SOUT_FELL; fall_steps = (float)(t - s); decided = true; return; }
        if (done > 0.0f || cmd[0] != c1[0] || cmd[1] != c1[1] || cmd[2] != c1[2]) { outcome = KBJ_SOUT_CENSORED; decided = true; return; }
      }
      // S_k(t): rows max(first, t - m + 1) .. t of this lane's ring column, ascending, in double, rounded once
      double sum[KBJ_NSCH] = {0.0, 0.0, 0.0};
      for (int u = t - m + 1; u <= t; ++u) {                   // m is uniform; a row in front of `first` is not this lane's: not added
        if (u < first) continue;
#pragma unroll
        for (int j = 0; j < KBJ_NSCH; ++j) sum[j] += (double)ring[u & (SR_RING - 1)][j][lane];
      }
      const double count = (double)(t - max(first, t - m + 1) + 1);
      float S[KBJ_NSCH];
#pragma unroll
      for (int j = 0; j < KBJ_NSCH; ++j) S[j] = (float)(sum[j] / count);
      if (t < s) {                                             // t == s - 1: was the robot on its old command?
        bool on = true;
#pragma unroll
        for (int j = 0; j < KBJ_NSCH; ++j) on = on && fabsf(__fsub_rn(S[j], c0[j])) <= band[j];
        if (!on) decided = true;                               // stays VOID
        return;
      }
      bool within = true;
#pragma unroll
      for (int j = 0; j < KBJ_NSCH; ++j) {
        const float d = __fsub_rn(S[j], c1[j]), p0 = __fsub_rn(S[j], c0[j]);
        const float sd = neg[j] ? -d : d, p = neg[j] ? -p0 : p0;
        if (act[j]) {
          if (rise[j] < 0.0f && p >= thr[j]) rise[j] = (float)(t - s);
          over[j] = sr_max(over[j], sd);
        } else {
          dev[j] = sr_max(dev[j], fabsf(d));
        }
        travel[j] += (double)v[j];
        within = within && fabsf(d) <= band[j];
      }
      run = within ? run + 1 : 0;
      if (run >= hold) { outcome = KBJ_SOUT_SETTLED; settle_steps = (float)((t - hold + 1) - s); decided = true; }
    });
  if (!decided) outcome = w.end64 > (long long)T ? KBJ_SOUT_CENSORED : KBJ_SOUT_UNSETTLED;    // the rows in front passed, the window ran out
  const bool valid = outcome >= KBJ_SOUT_FELL;
  if (live) {
    float4* o = reinterpret_cast<float4*>(rec + (size_t)env * KBJ_SREC_SIZE);
    float f[KBJ_SREC_SIZE];
#pragma unroll
    for (int k = 0; k < KBJ_SREC_SIZE; ++k) f[k] = -1.0f;
    f[KBJ_SREC_OUTCOME] = (float)outcome;
    if (valid) {
      f[KBJ_SREC_SETTLE_STEPS] = settle_steps; f[KBJ_SREC_FALL_STEPS] = fall_steps; f[KBJ_SREC_ACTIVE] = (float)active;
#pragma unroll
      for (int k = 0; k < KBJ_NSCH; ++k) {
        f[KBJ_SREC_TRAVEL_X + k] = (float)travel[k];
        f[KBJ_SREC_RISE + k] = act[k] ? rise[k] : -1.0f;
        f[KBJ_SREC_OVER + k] = act[k] ? over[k] : -1.0f;
        f[KBJ_SREC_DEV + k] = act[k] ? -1.0f : dev[k];
      }
    }
    f[KBJ_SREC_SPARE] = 0.0f;
#pragma unroll
    for (int k = KBJ_SREC_SPARE_TAIL; k < KBJ_SREC_SIZE; ++k) f[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < KBJ_SREC_SIZE / 4; ++k) o[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
  }
}

// one workgroup of GROUP_REDUCE_THREADS; thread g < G: group g's statistics over the envs in env order -> stats [G][KBJ_SSTAT_SIZE]. group == null: every
// env is in group 0; an env whose group is outside [0, G) is in none.
__global__ __launch_bounds__(GROUP_REDUCE_THREADS) void step_reduce_kernel(const float* __restrict__ rec, const int32_t* __restrict__ group, int N, int G,
                                                                      double* __restrict__ stats) {
  __shared__ __align__(16) float row[GROUP_REDUCE_THREADS][KBJ_SREC_SIZE];
  __shared__ int grp[GROUP_REDUCE_THREADS];
  const int g = threadIdx.x;
  int cnt[KBJ_SOUT_COUNT] = {0, 0, 0, 0, 0, 0}, an[KBJ_NSCH] = {0, 0, 0}, rn[KBJ_NSCH] = {0, 0, 0}, dn[KBJ_NSCH] = {0, 0, 0};
  double ss = 0, sq = 0, sm = -1, fs = 0, fq = 0, fm = -1;
  double rs[KBJ_NSCH] = {0, 0, 0}, rm[KBJ_NSCH] = {-1, -1, -1}, os[KBJ_NSCH] = {0, 0, 0}, om[KBJ_NSCH] = {-1, -1, -1};
  double ds[KBJ_NSCH] = {0, 0, 0}, dm[KBJ_NSCH] = {-1, -1, -1}, ts[KBJ_NSCH] = {0, 0, 0}, tm[KBJ_NSCH] = {-1, -1, -1};
  for (int n0 = 0; n0 < N; n0 += GROUP_REDUCE_THREADS) {
    const int nb = min(GROUP_REDUCE_THREADS, N - n0);
    group_stage_round(row, grp, rec, group, n0, nb);
    if (g < G) {
      for (int i = 0; i < nb; ++i) {
        if (grp[i] != g) continue;
        const float* r = row[i];
        const int oc = (int)r[KBJ_SREC_OUTCOME];
#pragma unroll
        for (int k = 0; k < KBJ_SOUT_COUNT; ++k) cnt[k] += oc == k;
        if (oc == KBJ_SOUT_SETTLED) { const double x = (double)r[KBJ_SREC_SETTLE_STEPS]; ss += x; sq += x * x; sm = sr_max(sm, x); }
        if (oc == KBJ_SOUT_FELL) { const double x = (double)r[KBJ_SREC_FALL_STEPS]; fs += x; fq += x * x; fm = sr_max(fm, x); }
        if (oc >= KBJ_SOUT_FELL) {
          const int active = (int)r[KBJ_SREC_ACTIVE];
#pragma unroll
          for (int k = 0; k < KBJ_NSCH; ++k) {
            if (active >> k & 1) {
              const double rise = (double)r[KBJ_SREC_RISE + k], ov = (double)r[KBJ_SREC_OVER + k];
              an[k] += 1;
              if (rise >= 0.0) { rn[k] += 1; rs[k] += rise; rm[k] = sr_max(rm[k], rise); }
              os[k] += ov; om[k] = sr_max(om[k], ov);
            } else {
              const double dv = (double)r[KBJ_SREC_DEV + k];
              dn[k] += 1; ds[k] += dv; dm[k] = sr_max(dm[k], dv);
            }
          }
        }
        if (oc == KBJ_SOUT_SETTLED) {
#pragma unroll
          for (int k = 0; k < KBJ_NSCH; ++k) { const double x = (double)r[KBJ_SREC_TRAVEL_X + k]; ts[k] += x; tm[k] = sr_max(tm[k], fabs(x)); }
        }
      }
    }
  }
  if (g < G) {
    double* o = stats + (size_t)g * KBJ_SSTAT_SIZE;
#pragma unroll
    for (int k = 0; k < KBJ_SOUT_COUNT; ++k) o[KBJ_SSTAT_COUNT + k] = (double)cnt[k];
    o[KBJ_SSTAT_SETTLE_SUM] = ss; o[KBJ_SSTAT_SETTLE_SUMSQ] = sq; o[KBJ_SSTAT_SETTLE_MAX] = sm;
    o[KBJ_SSTAT_FALL_SUM] = fs; o[KBJ_SSTAT_FALL_SUMSQ] = fq; o[KBJ_SSTAT_FALL_MAX] = fm;
#pragma unroll
    for (int k = 0; k < KBJ_NSCH; ++k) {
      o[KBJ_SSTAT_ACTIVE_N + k] = (double)an[k]; o[KBJ_SSTAT_RISE_N + k] = (double)rn[k]; o[KBJ_SSTAT_RISE_SUM + k] = rs[k]; o[KBJ_SSTAT_RISE_MAX + k] = rm[k];
      o[KBJ_SSTAT_OVER_SUM + k] = os[k]; o[KBJ_SSTAT_OVER_MAX + k] = om[k];
      o[KBJ_SSTAT_DEV_N + k] = (double)dn[k]; o[KBJ_SSTAT_DEV_SUM + k] = ds[k]; o[KBJ_SSTAT_DEV_MAX + k] = dm[k];
      o[KBJ_SSTAT_TRAVEL_SUM + k] = ts[k]; o[KBJ_SSTAT_TRAVEL_ABSMAX + k] = tm[k];
    }
    for (int k = KBJ_SSTAT_TRAVEL_ABSMAX + KBJ_NSCH; k < KBJ_SSTAT_SIZE; ++k) o[k] = 0.0;
  }
}

}  // namespace
}  // namespace kbj
