// kbj_frequency_response.h — how the robot follows a stick that keeps moving (kbj_frequency_response): on kbj_step_response's signal (stage 1 is
// step_signal_kernel itself, launched by the entry point through the same helper), per env the lock-in sums of ONE scheduled window of whole
// periods - the three response channels against the driven command word and against the same word a quarter period earlier (KBJ_FOUT_*,
// KBJ_FREC_*) - then per group of envs their ordered pooled sums (KBJ_FSTAT_*). The rule is in include/kbj.h at kbj_frequency_response, word for
// word; tests/frequency_response_ref.py restates it; gain, lag, delay and coherence are host arithmetic on the sums (host/frequency.py). Included
// by kbj_traj_stats.hip.
//
// Shapes.
// freq_scan_kernel: window_walk (kbj_window_scan.h) over chunks of FR_TC rows with hold = q = P / 4 lead rows in front of s; the schedule row
// {s, P, ch, K} is one 16-byte load per lane. The delayed reference d(t) = r(t - q) has a per-lane delay of up to 64 rows: as a register array it
// would be indexed dynamically, that is scratch, so it is an LDS ring [64][64] floats = 16 KB with the lane as the fastest index. A lane reads
// slot (t - q) & 63 and THEN writes slot t & 63 (at q = 64 they are the same slot); it only ever reads words it wrote itself on an earlier row
// of its own window (the lead rows [s - q, s) are walked for that), so there is no barrier. Whatever a lane's q, lane l touches bank l & 31: each
// half-wave covers the 32 banks once. r is chosen by two selects on ch, not by an indexed read of the row. 17 double accumulators = 34 VGPRs.
// Second stage (when stats are asked for): freq_reduce_kernel, the group reduce of kbj_window_scan.h on records of 24 doubles staged as 48 floats.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "kbj.h"
#include "kbj_window_scan.h"
#include "kbj_step_response.h"   // SrRow, the signal row as the scan fetches it

namespace kbj {
namespace {

constexpr int FR_TC = 4;          // rows per chunk: 8 registers a row, two images
constexpr int FR_RING = 64;       // rows of the delay ring = the largest quarter period
constexpr int FR_MAX_PERIOD = 4 * FR_RING;
constexpr int FR_REC_FLOATS = 2 * KBJ_FREC_SIZE;   // a record of doubles as the group reduce stages it
static_assert(FR_MAX_PERIOD == 256, "the period range kbj.h documents: [4, 256]");
static_assert((FR_RING & (FR_RING - 1)) == 0, "ring slots are taken with a mask");
static_assert(KBJ_FREC_SIZE == 24 && KBJ_FREC_S_R == 7 && KBJ_FREC_S_Y == 12 && KBJ_FREC_S_YY == 15 && KBJ_FREC_S_YR == 18 && KBJ_FREC_S_YD == 21, "a record row: 7 head words, 5 reference sums, 4 x 3 response sums");
static_assert(KBJ_FREC_S_R + KBJ_FREC_NSUMS == KBJ_FREC_SIZE && FR_REC_FLOATS % 4 == 0, "the sums close the record; it is staged as 16-byte pieces");
static_assert(KBJ_FOUT_COUNT == KBJ_FSTAT_FALL_SUM - KBJ_FSTAT_COUNT && KBJ_FSTAT_SUMS + KBJ_FREC_NSUMS == KBJ_FSTAT_R_MIN && KBJ_FSTAT_R_MAX < KBJ_FSTAT_SIZE, "frequency statistics layout");

// grid = ceil(N / 64) workgroups of one wavefront; sig [T][N][KBJ_SSIG_SIZE], sched [N][4] (16-byte aligned), rec [N][KBJ_FREC_SIZE] doubles
__global__ __launch_bounds__(WINDOW_ENVS) void freq_scan_kernel(const float* __restrict__ sig, int T, int N, const int32_t* __restrict__ sched, kbj_frequency_criteria crit,
                                                                 double* __restrict__ rec) {
  __shared__ float ring[FR_RING][WINDOW_ENVS];
  const int lane = threadIdx.x, env = blockIdx.x * WINDOW_ENVS + lane;
  const bool live = env < N;
  const int4 sc = live ? reinterpret_cast<const int4*>(sched)[env] : make_int4(-1, 0, 0, 0);
  const int s = sc.x, P = sc.y, ch = sc.z, K = sc.w;
  const bool sound = P >= 4 && P <= FR_MAX_PERIOD && P % 4 == 0 && ch >= 0 && ch <= 2 && K >= 1;
  const int q = sound ? P / 4 : 0;
  const Window w(live && s >= 0 && sound, s, q, sound ? (long long)K * (long long)P : 0ll, T);     // K, P >= 1: end > s for a scanned env

  int outcome = !live || s < 0 ? KBJ_FOUT_NONE : KBJ_FOUT_VOID;      // a scanned env: VOID until its lead rows have passed
  bool decided = !w.scan;
  int rows = 0;
  int fall_steps = -1;
  float rmin = INFINITY, rmax = -INFINITY;
  double sr = 0.0, sd = 0.0, srr = 0.0, sdd = 0.0, srd = 0.0;
  double sy[KBJ_NSCH] = {0.0, 0.0, 0.0}, syy[KBJ_NSCH] = {0.0, 0.0, 0.0}, syr[KBJ_NSCH] = {0.0, 0.0, 0.0}, syd[KBJ_NSCH] = {0.0, 0.0, 0.0};

  window_walk<FR_TC, SrRow>(w, decided,
    [&](SrRow& r, int t) {
      const float4* p = reinterpret_cast<const float4*>(sig + ((size_t)t * N + env) * KBJ_SSIG_SIZE);
      r.v = p[0]; r.c = p[1];
    },
    [&](const SrRow& row, int t) {
      const float c0 = row.c.x, c1 = row.c.y, c2 = row.c.z;      // loaded first: a conditional over the members selects an ADDRESS into the image, which keeps it in scratch
      const float r = ch == 0 ? c0 : ch == 1 ? c1 : c2;
      const float done = row.v.w;
      const float d = t >= s ? ring[(t - q) & (FR_RING - 1)][lane] : 0.0f;     // row t - q >= s - q: this lane wrote it; read before the write below
      ring[t & (FR_RING - 1)][lane] = r;
      if (t < s) {                                             // the lead rows
        if (done != 0.0f) decided = true;                      // stays VOID
        return;
      }
      if (done < 0.0f) { outcome = KBJ_FOUT_FELL; fall_steps = t - s; decided = true; return; }
      if (done > 0.0f) { outcome = KBJ_FOUT_CENSORED; decided = true; return; }
      rmin = r < rmin ? r : rmin;
      rmax = r > rmax ? r : rmax;
      rows += 1;
      const double rd = (double)r, dd = (double)d;
      const double y[KBJ_NSCH] = {(double)row.v.x, (double)row.v.y, (double)row.v.z};
      sr += rd; sd += dd; srr += rd * rd; sdd += dd * dd; srd += rd * dd;
#pragma unroll
      for (int k = 0; k < KBJ_NSCH; ++k) { sy[k] += y[k]; syy[k] += y[k] * y[k]; syr[k] += y[k] * rd; syd[k] += y[k] * dd; }
    });
  if (!decided) {                                              // the lead rows passed and no row stopped the scan
    const float a0 = crit.min_amp[0], a1 = crit.min_amp[1], a2 = crit.min_amp[2];
    const float amp = ch == 0 ? a0 : ch == 1 ? a1 : a2;
    outcome = w.end64 > (long long)T ? KBJ_FOUT_CENSORED : __fsub_rn(rmax, rmin) >= amp ? KBJ_FOUT_MEASURED : KBJ_FOUT_FLAT;
  }
  if (live) {
    double* o = rec + (size_t)env * KBJ_FREC_SIZE;             // 8-byte stores: rec_d is 8-byte aligned
    const bool valid = outcome >= KBJ_FOUT_FELL;
    o[KBJ_FREC_OUTCOME] = (double)outcome;
    o[KBJ_FREC_ROWS] = valid ? (double)rows : -1.0;
    o[KBJ_FREC_FALL_STEPS] = valid ? (double)fall_steps : -1.0;
    o[KBJ_FREC_CHANNEL] = valid ? (double)ch : -1.0;
    o[KBJ_FREC_PERIOD] = valid ? (double)P : -1.0;
    o[KBJ_FREC_R_MIN] = valid ? (double)rmin : -1.0;
    o[KBJ_FREC_R_MAX] = valid ? (double)rmax : -1.0;
    o[KBJ_FREC_S_R] = valid ? sr : -1.0; o[KBJ_FREC_S_D] = valid ? sd : -1.0; o[KBJ_FREC_S_RR] = valid ? srr : -1.0;
    o[KBJ_FREC_S_DD] = valid ? sdd : -1.0; o[KBJ_FREC_S_RD] = valid ? srd : -1.0;
#pragma unroll
    for (int k = 0; k < KBJ_NSCH; ++k) {
      o[KBJ_FREC_S_Y + k] = valid ? sy[k] : -1.0; o[KBJ_FREC_S_YY + k] = valid ? syy[k] : -1.0;
      o[KBJ_FREC_S_YR + k] = valid ? syr[k] : -1.0; o[KBJ_FREC_S_YD + k] = valid ? syd[k] : -1.0;
    }
  }
}

// one workgroup of GROUP_REDUCE_THREADS; thread g < G: group g's statistics over the envs in env order -> stats [G][KBJ_FSTAT_SIZE]. group == null: every
// env is in group 0; an env whose group is outside [0, G) is in none. rec [N][KBJ_FREC_SIZE] doubles, staged as FR_REC_FLOATS floats a record:
// group_stage_round moves 16-byte pieces, so a rec that is only 8-byte aligned (kbj.h asks no more) is staged in 8-byte pieces instead.
__global__ __launch_bounds__(GROUP_REDUCE_THREADS) void freq_reduce_kernel(const double* __restrict__ rec, const int32_t* __restrict__ group, int N, int G,
                                                                           double* __restrict__ stats) {
  __shared__ __align__(16) float row[GROUP_REDUCE_THREADS][FR_REC_FLOATS];
  __shared__ int grp[GROUP_REDUCE_THREADS];
  const int g = threadIdx.x;
  const bool wide = (reinterpret_cast<uintptr_t>(rec) & 15) == 0;      // uniform
  int cnt[KBJ_FOUT_COUNT] = {0, 0, 0, 0, 0, 0};
  double fs = 0.0, nrows = 0.0, rmin = INFINITY, rmax = -INFINITY;
  double sum[KBJ_FREC_NSUMS];
#pragma unroll
  for (int k = 0; k < KBJ_FREC_NSUMS; ++k) sum[k] = 0.0;
  for (int n0 = 0; n0 < N; n0 += GROUP_REDUCE_THREADS) {
    const int nb = min(GROUP_REDUCE_THREADS, N - n0);
    if (wide) {
      group_stage_round(row, grp, reinterpret_cast<const float*>(rec), group, n0, nb);
    } else {
      __syncthreads();                                         // the round before has been read
      for (int i = threadIdx.x; i < nb * KBJ_FREC_SIZE; i += GROUP_REDUCE_THREADS)
        reinterpret_cast<double*>(&row[0][0])[i] = rec[(size_t)n0 * KBJ_FREC_SIZE + i];
      if (threadIdx.x < nb) grp[threadIdx.x] = group ? group[n0 + threadIdx.x] : 0;
      __syncthreads();
    }
    if (g < G) {
      for (int i = 0; i < nb; ++i) {
        if (grp[i] != g) continue;
        const double* r = reinterpret_cast<const double*>(row[i]);
        const int oc = (int)r[KBJ_FREC_OUTCOME];
#pragma unroll
        for (int k = 0; k < KBJ_FOUT_COUNT; ++k) cnt[k] += oc == k;
        if (oc == KBJ_FOUT_FELL) fs += r[KBJ_FREC_FALL_STEPS];
        if (oc == KBJ_FOUT_MEASURED) {
          nrows += r[KBJ_FREC_ROWS];
#pragma unroll
          for (int k = 0; k < KBJ_FREC_NSUMS; ++k) sum[k] += r[KBJ_FREC_S_R + k];
          const double lo = r[KBJ_FREC_R_MIN], hi = r[KBJ_FREC_R_MAX];
          rmin = lo < rmin ? lo : rmin;
          rmax = hi > rmax ? hi : rmax;
        }
      }
    }
  }
  if (g < G) {
    double* o = stats + (size_t)g * KBJ_FSTAT_SIZE;
    const bool any = cnt[KBJ_FOUT_MEASURED] > 0;
#pragma unroll
    for (int k = 0; k < KBJ_FOUT_COUNT; ++k) o[KBJ_FSTAT_COUNT + k] = (double)cnt[k];
    o[KBJ_FSTAT_FALL_SUM] = fs; o[KBJ_FSTAT_ROWS] = nrows;
#pragma unroll
    for (int k = 0; k < KBJ_FREC_NSUMS; ++k) o[KBJ_FSTAT_SUMS + k] = sum[k];
    o[KBJ_FSTAT_R_MIN] = any ? rmin : -1.0; o[KBJ_FSTAT_R_MAX] = any ? rmax : -1.0;
    for (int k = KBJ_FSTAT_R_MAX + 1; k < KBJ_FSTAT_SIZE; ++k) o[k] = 0.0;
  }
}

}  // namespace
}  // namespace kbj
