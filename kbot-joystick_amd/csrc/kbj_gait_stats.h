// kbj_gait_stats.h — the contact pattern of one trajectory (kbj_gait_stats): swing and stance durations, support shares, foot clearance, hops,
// ground force and torque level, split by the command mode of the row (KBJ_GACC_*, KBJ_GAIT_*, KBJ_GFOOT_*, KBJ_GENV_*). Included by
// kbj_traj_stats.hip.
//
// One-row skew, by definition: KBJ_AUX_TOUCH is the observation the policy saw BEFORE the step, KBJ_AUX_LFZ / _RFZ are the foot heights AFTER
// it. The contact bit of row t therefore belongs to the state that row t - 1 left, the heights to the state row t leaves. rewards_kernel reads
// the same columns the same way; nothing here corrects it.
//
// Shape: tracking_stats_kernel's. One workgroup of five wavefronts owns 32 consecutive envs. Wavefronts 1-4 each fetch one time step of a
// 4-step chunk as coalesced 16-byte pieces (one chunk ahead, so the loads fly under the evaluation and the scan of the chunk before), put the
// 13 pieces that are read (LFZ / RFZ, CTRL, TOUCH, CMD, DONE) into LDS (kbj_aux_stage.h: a row stride of 53 words) and evaluate there, one env per lane, everything of a row that does not depend on the row before: the contact bits, the
// mode, DONE, q = sum ctrl^2 and qmax = max |ctrl|. What is left per row is six words and one double. Wavefront 0 runs the ordered part from
// them, one env per lane: phases, events, clearance.
// The per-mode accumulators are indexed by a run-time mode, so they do not live in registers (they would become scratch): they are two LDS
// images with the lane as the fastest index. A row is 32 words or 32 doubles, so the 32 lanes fall on 32 different banks (b32) or 64 (b64)
// whatever mode each lane holds: conflict-free read-modify-writes.
// Envs per workgroup: 32, in the lower half of every wavefront. The scan is serial in t, so its time does not depend on how many lanes it
// fills; at 8192 envs 64 per workgroup would leave half of the 256 CUs without a workgroup (measured: 213 us against 190 us, EXPERIMENTS.md
// "Gait statistics"), and at 74 KB two workgroups share a CU when there are more.
// What needs a double and what does not. All 39 used slots of the 6 mode blocks as doubles would be 59 KB. A lane's own counts and duration
// sums are whole numbers below 2^32 within one call (a duration is at most 2^24 rows, and only the first phase a foot ends in a call can be
// longer than the call), and its maxima are fp32 values: those 28 slots per mode are 32-bit words (21 KB; counts as uint32, maxima as float).
// Doubles are kept for the 11 slots per mode that are real-valued sums or sums of squares of durations (up to 2^48): TORQUE_SQ and per foot
// SWING_SUMSQ, STANCE_SUMSQ, CLEAR_SUM, CLEAR_SUMSQ, FORCE_SUM (17 KB). With four staged time steps (27 KB) and two chunks of evaluated rows
// (8 KB) the kernel holds 73,856 bytes of LDS.
// Lanes are combined in lane order, in double, the workgroup partials in block order by kbj_ordered_reduce.h over GaitSlots: fixed order, no
// atomics - a call is bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "kbj_model.h"
#include "kbj_aux_stage.h"
#include "kbj_ordered_reduce.h"

namespace kbj {
namespace {

constexpr int GAIT_ENVS = 32;        // envs per workgroup: the lower half of every wavefront's lanes holds one env each
constexpr int GAIT_TC = 4;           // time steps per chunk: one per staging wavefront
constexpr int GAIT_THREADS = 64 * (GAIT_TC + 1);   // wavefront 0 scans, wavefronts 1-4 stage and evaluate
constexpr int GAIT_KL = GAIT_ENVS * AUX_V4 / 64;   // pieces per lane and time step
constexpr int GAIT_RES = 6;          // words per evaluated row: flags, z[2], F[2], qmax
constexpr float GAIT_CONTACT_FORCE = 0.1f;         // rewards_kernel's contact test: TOUCH > 0.1f
constexpr float GAIT_RUN_CAP = 16777216.0f;        // 2^24: the last fp32 a + 1 still counts up to

// the kind of a foot slot: a 32-bit count (0), an fp32 maximum (1), a double sum (2)
__host__ __device__ constexpr int gait_foot_kind(int k) {
  return (k == KBJ_GFOOT_SWING_MAX || k == KBJ_GFOOT_STANCE_MAX || k == KBJ_GFOOT_CLEAR_MAX || k == KBJ_GFOOT_FORCE_MAX) ? 1
       : (k == KBJ_GFOOT_SWING_SUMSQ || k == KBJ_GFOOT_STANCE_SUMSQ || k == KBJ_GFOOT_CLEAR_SUM || k == KBJ_GFOOT_CLEAR_SUMSQ || k == KBJ_GFOOT_FORCE_SUM) ? 2 : 0;
}
// the index of foot slot k among the foot's words (kinds 0, 1) or among its doubles (kind 2)
__host__ __device__ constexpr int gait_foot_index(int k) {
  int n = 0;
  for (int j = 0; j < k; ++j) n += (gait_foot_kind(j) == 2) == (gait_foot_kind(k) == 2);
  return n;
}
constexpr int GAIT_FOOT_WORDS = gait_foot_index(KBJ_GFOOT_CONTACT_ROWS) + 1;    // 11
constexpr int GAIT_FOOT_DBLS = gait_foot_index(KBJ_GFOOT_FORCE_SUM) + 1;        // 5
constexpr int GAIT_ROW_WORDS = 6;    // ROWS, DOUBLE, SINGLE, FLIGHT, REPEATS, TORQUE_MAX
constexpr int GAIT_MODE_WORDS = GAIT_ROW_WORDS + 2 * GAIT_FOOT_WORDS;           // 28 rows of the word image per mode
constexpr int GAIT_MODE_DBLS = 1 + 2 * GAIT_FOOT_DBLS;                          // 11 rows of the double image per mode: TORQUE_SQ, then the feet
// rows inside a mode block of the two images
constexpr int GAIT_W_TORQUE_MAX = 5;                                            // the other row words sit at their KBJ_GAIT_* slot
__host__ __device__ constexpr int gait_w(int f, int k) { return GAIT_ROW_WORDS + GAIT_FOOT_WORDS * f + gait_foot_index(k); }
__host__ __device__ constexpr int gait_d(int f, int k) { return 1 + GAIT_FOOT_DBLS * f + gait_foot_index(k); }

static_assert(GAIT_ENVS <= 64 && GAIT_ENVS * AUX_V4 % 64 == 0 && KBJ_AUX_SIZE % 4 == 0 && KBJ_GACC_SIZE == 16 && KBJ_GACC_FOOT_STRIDE == 6 && KBJ_GACC_RUNNING == 12 && KBJ_GACC_LAST_TD == 13, "gait carry layout: four 16-byte pieces");
static_assert(GAIT_FOOT_WORDS == 11 && GAIT_FOOT_DBLS == 5 && GAIT_FOOT_WORDS + GAIT_FOOT_DBLS == KBJ_GFOOT_SIZE && KBJ_GFOOT_SIZE == KBJ_GAIT_FOOT_STRIDE, "foot block");
static_assert(KBJ_GAIT_REPEATS == 4 && KBJ_GAIT_TORQUE_SQ == 5 && KBJ_GAIT_TORQUE_MAX == 6 && KBJ_GAIT_FOOT == 8 && KBJ_GAIT_FOOT + 2 * KBJ_GAIT_FOOT_STRIDE == KBJ_GAIT_MODE_STRIDE &&
              KBJ_CMODE_COUNT * KBJ_GAIT_MODE_STRIDE == KBJ_GAIT_EPISODES && KBJ_GAIT_EPISODES < KBJ_GAIT_SIZE && KBJ_GAIT_SIZE <= GAIT_THREADS, "gait statistics layout");
static_assert(KBJ_GENV_FOOT == 8 && KBJ_GENV_FOOT + 2 * KBJ_GENV_FOOT_STRIDE == KBJ_GENV_SIZE && KBJ_GENV_SIZE % 4 == 0, "per-env record layout");

// the staged pieces of an aux row (kbj_aux_stage.h): those read are 2-3 (LFZ, RFZ) and 7-17 (CTRL, TOUCH, CMD, DONE)
struct GaitMap {
  static constexpr int NPIECE = 13;
  static __device__ constexpr int piece(int p) { return (p == 2 || p == 3) ? p - 2 : (p >= 7 && p <= 17) ? p - 5 : -1; }
};
using GaitRow = StagedRow<GaitMap>;
constexpr int GAIT_LD = GaitRow::LD;
static_assert(GaitMap::piece(KBJ_AUX_LFZ / 4) == 0 && GaitMap::piece(KBJ_AUX_RFZ / 4) == 1 && GaitMap::piece(KBJ_AUX_CTRL / 4) == 2 && GaitMap::piece((KBJ_AUX_CTRL + KBJ_NU - 1) / 4) >= 2 &&
              GaitMap::piece((KBJ_AUX_TOUCH + 1) / 4) >= 2 && GaitMap::piece(KBJ_AUX_CMD / 4) >= 2 && GaitMap::piece(KBJ_AUX_DONE / 4) == GaitMap::NPIECE - 1 && GaitMap::piece(1) == -1 &&
              GaitMap::piece(6) == -1 && GAIT_LD == 53 && KBJ_AUX_SIZE / 4 == 18 && KBJ_AUX_CTRL / 4 == 7, "staged pieces");

struct GaitShared {
  double dimg[KBJ_CMODE_COUNT * GAIT_MODE_DBLS][GAIT_ENVS];     // [mode * GAIT_MODE_DBLS + row][lane]
  uint32_t wimg[KBJ_CMODE_COUNT * GAIT_MODE_WORDS][GAIT_ENVS];  // [mode * GAIT_MODE_WORDS + row][lane]: counts as uint32, maxima as float bits
  double q[2][GAIT_TC][GAIT_ENVS];                              // sum ctrl^2 of the rows of chunk c in q[c & 1]
  float res[2][GAIT_TC][GAIT_RES][GAIT_ENVS];                   // evaluated rows of chunk c in res[c & 1]: [tt][flags | z | F | qmax][env]
  float raw[GAIT_TC][GAIT_ENVS * GAIT_LD];                      // the chunk's aux rows, [tt][env * GAIT_LD + column]
  uint32_t episodes[GAIT_ENVS];                                 // episodes each lane started
};
static_assert(sizeof(GaitShared) <= 160 * 1024, "one workgroup per CU");

// the slots of a KBJ_GAIT vector (kbj_ordered_reduce.h): counts and sums, but for the maxima of each mode block (each of a non-negative
// quantity)
struct GaitSlots : SumMaxSlots<GaitSlots> {
  static constexpr int SIZE = KBJ_GAIT_SIZE;
  static __device__ inline bool is_max(int j) {
    if (j >= KBJ_GAIT_EPISODES) return false;
    const int s = j % KBJ_GAIT_MODE_STRIDE;
    return s == KBJ_GAIT_TORQUE_MAX || (s >= KBJ_GAIT_FOOT && gait_foot_kind((s - KBJ_GAIT_FOOT) % KBJ_GAIT_FOOT_STRIDE) == 1);
  }
};

// accessors of one lane's cells of a mode block
struct GaitCells {
  double (*D)[GAIT_ENVS];
  uint32_t (*W)[GAIT_ENVS];
  int lane;
  __device__ void count(int row, uint32_t by = 1u) const { W[row][lane] += by; }
  __device__ void fmax_(int row, float x) const { W[row][lane] = __float_as_uint(fmaxf(__uint_as_float(W[row][lane]), x)); }
  __device__ void add(int row, double x) const { D[row][lane] += x; }
};

// grid = ceil(N / 32) workgroups of 320 threads; part_out [gridDim.x][KBJ_GAIT_SIZE]; env_out [N][KBJ_GENV_SIZE] or null
__global__ __launch_bounds__(GAIT_THREADS) void gait_stats_kernel(const float* __restrict__ aux, int T, int N, float* __restrict__ acc, double* __restrict__ part_out,
                                                                  float* __restrict__ env_out) {
  __shared__ __align__(16) GaitShared S;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int e0 = blockIdx.x * GAIT_ENVS, nb = min(GAIT_ENVS, N - e0);
  const int nchunk = (T + GAIT_TC - 1) / GAIT_TC;
  const int npiece = nb * AUX_V4;                 // 16-byte pieces of the block's rows of one time step
  const bool live = lane < nb;

  for (int i = tid; i < KBJ_CMODE_COUNT * GAIT_MODE_DBLS * GAIT_ENVS; i += GAIT_THREADS) (&S.dimg[0][0])[i] = 0.0;
  for (int i = tid; i < KBJ_CMODE_COUNT * GAIT_MODE_WORDS * GAIT_ENVS; i += GAIT_THREADS) (&S.wimg[0][0])[i] = 0u;    // 0.0f as well
  if (tid < GAIT_ENVS) S.episodes[tid] = 0u;

  // scanner state (wavefront 0): the env's carry row, and its totals of this call over all modes (the per-env record)
  float con[2] = {0, 0}, run[2] = {0, 0}, valid[2] = {0, 0}, zst[2] = {0, 0}, peak[2] = {0, 0}, spare[4] = {0, 0, 0, 0}, running = 0, last_td = 0;
  uint32_t n_rows = 0, n_support[3] = {0, 0, 0}, n_repeats = 0, n_episodes = 0, n_td[2] = {0, 0}, n_swing[2] = {0, 0}, swing_sum[2] = {0, 0}, n_stance[2] = {0, 0}, stance_sum[2] = {0, 0};
  double torque_sq = 0, clear_sum[2] = {0, 0};
  float torque_max = 0, clear_max[2] = {0, 0}, force_max[2] = {0, 0};
  float4* row = reinterpret_cast<float4*>(acc + (size_t)(e0 + lane) * KBJ_GACC_SIZE);
  if (live && wave == 0) {
    const float4 a0 = row[0], a1 = row[1], a2 = row[2], a3 = row[3];
    con[0] = a0.x; run[0] = a0.y; valid[0] = a0.z; zst[0] = a0.w; peak[0] = a1.x; spare[0] = a1.y;
    con[1] = a1.z; run[1] = a1.w; valid[1] = a2.x; zst[1] = a2.y; peak[1] = a2.z; spare[1] = a2.w;
    running = a3.x; last_td = a3.y; spare[2] = a3.z; spare[3] = a3.w;
  }

  // staging registers: the pieces lane, lane + 64, ... of time step c * GAIT_TC + wave - 1, those that are read
  float4 v[GAIT_KL];
  auto fetch = [&](int c) {
    const int t = c * GAIT_TC + wave - 1;
    if (wave == 0 || t >= T) return;
    const float4* src = reinterpret_cast<const float4*>(aux + ((size_t)t * N + e0) * KBJ_AUX_SIZE);
#pragma unroll
    for (int k = 0; k < GAIT_KL; ++k) {
      const int i = k * 64 + lane;
      if (i < npiece && GaitMap::piece(i % AUX_V4) >= 0) v[k] = src[i];
    }
  };
  fetch(0);

  for (int c = 0; c <= nchunk; ++c) {
    const int tt = wave - 1, t = c * GAIT_TC + tt;
    const bool mine = wave > 0 && c < nchunk && t < T;     // this wavefront has a time step in chunk c
    if (mine) {
#pragma unroll
      for (int k = 0; k < GAIT_KL; ++k) stage_piece<GaitMap>(S.raw[tt], v[k], k * 64 + lane, npiece);
    }
    __syncthreads();
    if (wave > 0) {
      if (c + 1 < nchunk) fetch(c + 1);                    // the next chunk's loads fly under the evaluation and the scan
      if (mine && live) {
        const GaitRow a{S.raw[tt] + lane * GAIT_LD};
        const float F0 = a[KBJ_AUX_TOUCH], F1 = a[KBJ_AUX_TOUCH + 1];
        double q = 0.0;
        float qmax = 0.0f;
#pragma unroll
        for (int u = 0; u < KBJ_NU; ++u) { const float x = a[KBJ_AUX_CTRL + u]; q += (double)x * (double)x; qmax = fmaxf(qmax, fabsf(x)); }
        const int flags = cmd_mode(a) | (F0 > GAIT_CONTACT_FORCE ? 8 : 0) | (F1 > GAIT_CONTACT_FORCE ? 16 : 0) | (a[KBJ_AUX_DONE] == 0.0f ? 32 : 0);
        float (*r)[GAIT_ENVS] = S.res[c & 1][tt];
        r[0][lane] = __int_as_float(flags);
        r[1][lane] = a[KBJ_AUX_LFZ]; r[2][lane] = a[KBJ_AUX_RFZ];
        r[3][lane] = F0; r[4][lane] = F1; r[5][lane] = qmax;
        S.q[c & 1][tt][lane] = q;
      }
    } else if (live && c > 0) {      // ordered scan of chunk c - 1
      const int tc = min(GAIT_TC, T - (c - 1) * GAIT_TC);
      for (int s = 0; s < tc; ++s) {
        const float (*r)[GAIT_ENVS] = S.res[(c - 1) & 1][s];
        const int flags = __float_as_int(r[0][lane]), mode = flags & 7;
        const bool cn[2] = {(flags & 8) != 0, (flags & 16) != 0};
        const float z[2] = {r[1][lane], r[2][lane]}, F[2] = {r[3][lane], r[4][lane]}, qmax = r[5][lane];
        const double q = S.q[(c - 1) & 1][s][lane];
        const GaitCells A{S.dimg + mode * GAIT_MODE_DBLS, S.wimg + mode * GAIT_MODE_WORDS, lane};
        // 1. the row
        const int support = 2 - (int)cn[0] - (int)cn[1];       // 0 double, 1 single, 2 flight
        A.count(KBJ_GAIT_ROWS); A.count(KBJ_GAIT_DOUBLE + support);
        A.add(0, q); A.fmax_(GAIT_W_TORQUE_MAX, qmax);
        n_rows += 1; n_support[0] += support == 0; n_support[1] += support == 1; n_support[2] += support == 2;
        torque_sq += q; torque_max = fmaxf(torque_max, qmax);
        // 2. contact rows and ground force
#pragma unroll
        for (int f = 0; f < 2; ++f)
          if (cn[f]) {
            A.count(gait_w(f, KBJ_GFOOT_CONTACT_ROWS)); A.add(gait_d(f, KBJ_GFOOT_FORCE_SUM), (double)F[f]); A.fmax_(gait_w(f, KBJ_GFOOT_FORCE_MAX), F[f]);
            force_max[f] = fmaxf(force_max[f], F[f]);
          }
        if (running == 0.0f) {     // 3. the row starts an episode: no events
          n_episodes += 1;
#pragma unroll
          for (int f = 0; f < 2; ++f) { con[f] = cn[f] ? 1.0f : 0.0f; run[f] = 1.0f; valid[f] = 0.0f; zst[f] = z[f]; peak[f] = 0.0f; }
          last_td = -1.0f;
        } else {                   // 4. phases and events
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            if (cn[f] == (con[f] != 0.0f)) { run[f] = fminf(run[f] + 1.0f, GAIT_RUN_CAP); continue; }
            const bool counted = valid[f] != 0.0f;
            const uint32_t n = (uint32_t)run[f];
            const double nn = (double)run[f] * (double)run[f];
            if (cn[f]) {           // touchdown: a swing ends
              A.count(gait_w(f, KBJ_GFOOT_TOUCHDOWNS)); n_td[f] += 1;
              if (counted) {
                A.count(gait_w(f, KBJ_GFOOT_SWING_N)); A.count(gait_w(f, KBJ_GFOOT_SWING_SUM), n); A.add(gait_d(f, KBJ_GFOOT_SWING_SUMSQ), nn); A.fmax_(gait_w(f, KBJ_GFOOT_SWING_MAX), run[f]);
                const double p = (double)peak[f];
                A.add(gait_d(f, KBJ_GFOOT_CLEAR_SUM), p); A.add(gait_d(f, KBJ_GFOOT_CLEAR_SUMSQ), p * p); A.fmax_(gait_w(f, KBJ_GFOOT_CLEAR_MAX), peak[f]);
                n_swing[f] += 1; swing_sum[f] += n; clear_sum[f] += p; clear_max[f] = fmaxf(clear_max[f], peak[f]);
              }
              if (last_td == (float)f) { A.count(KBJ_GAIT_REPEATS); n_repeats += 1; }
              last_td = (float)f;
            } else {               // lift-off: a stance ends
              A.count(gait_w(f, KBJ_GFOOT_LIFTOFFS));
              if (counted) {
                A.count(gait_w(f, KBJ_GFOOT_STANCE_N)); A.count(gait_w(f, KBJ_GFOOT_STANCE_SUM), n); A.add(gait_d(f, KBJ_GFOOT_STANCE_SUMSQ), nn); A.fmax_(gait_w(f, KBJ_GFOOT_STANCE_MAX), run[f]);
                n_stance[f] += 1; stance_sum[f] += n;
              }
            }
            con[f] = cn[f] ? 1.0f : 0.0f; run[f] = 1.0f; valid[f] = 1.0f; peak[f] = 0.0f;
          }
        }
        // 5. the height of the last contact row, the rise over it
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          if (cn[f]) zst[f] = z[f];
          else peak[f] = fmaxf(peak[f], z[f] - zst[f]);
        }
        running = (flags & 32) ? 1.0f : 0.0f;     // 6.
      }
    }
    __syncthreads();
  }

  if (wave == 0) {
    if (live) {
      row[0] = make_float4(con[0], run[0], valid[0], zst[0]); row[1] = make_float4(peak[0], spare[0], con[1], run[1]);
      row[2] = make_float4(valid[1], zst[1], peak[1], spare[1]); row[3] = make_float4(running, last_td, spare[2], spare[3]);
      if (env_out) {
        float4* o = reinterpret_cast<float4*>(env_out + (size_t)(e0 + lane) * KBJ_GENV_SIZE);
        o[0] = make_float4((float)n_rows, (float)n_support[0], (float)n_support[1], (float)n_support[2]);
        o[1] = make_float4((float)n_repeats, (float)torque_sq, torque_max, 0.0f);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          o[2 + 2 * f] = make_float4((float)n_td[f], (float)n_swing[f], (float)swing_sum[f], (float)n_stance[f]);
          o[3 + 2 * f] = make_float4((float)stance_sum[f], (float)clear_sum[f], clear_max[f], force_max[f]);
        }
      }
    }
    if (lane < GAIT_ENVS) S.episodes[lane] = n_episodes;     // lanes beyond the last env hold 0
  }
  __syncthreads();
  if (tid < KBJ_GAIT_SIZE) {         // slot tid of the partial: the lanes in lane order
    const int mode = tid / KBJ_GAIT_MODE_STRIDE, s = tid % KBJ_GAIT_MODE_STRIDE;
    // kind of the slot (0 count, 1 maximum, 2 double sum, -1 unused) and its row in the image of that kind
    int kind = -1, r = 0;
    if (tid == KBJ_GAIT_EPISODES) kind = 3;
    else if (tid < KBJ_GAIT_EPISODES) {
      if (s < KBJ_GAIT_TORQUE_SQ) { kind = 0; r = s; }
      else if (s == KBJ_GAIT_TORQUE_SQ) { kind = 2; r = 0; }
      else if (s == KBJ_GAIT_TORQUE_MAX) { kind = 1; r = GAIT_W_TORQUE_MAX; }
      else if (s >= KBJ_GAIT_FOOT) {
        const int f = (s - KBJ_GAIT_FOOT) / KBJ_GAIT_FOOT_STRIDE, k = (s - KBJ_GAIT_FOOT) % KBJ_GAIT_FOOT_STRIDE;
        kind = gait_foot_kind(k);
        r = (kind == 2 ? 1 + GAIT_FOOT_DBLS * f : GAIT_ROW_WORDS + GAIT_FOOT_WORDS * f) + gait_foot_index(k);
      }
    }
    double x = 0.0;
    if (kind == 3) {
      for (int l = 0; l < GAIT_ENVS; ++l) x += (double)S.episodes[l];
    } else if (kind == 2) {
      const double* p = S.dimg[mode * GAIT_MODE_DBLS + r];
      x = p[0];
      for (int l = 1; l < GAIT_ENVS; ++l) x += p[l];
    } else if (kind == 1) {
      const uint32_t* p = S.wimg[mode * GAIT_MODE_WORDS + r];
      for (int l = 0; l < GAIT_ENVS; ++l) x = GaitSlots::combine_as(true, x, (double)__uint_as_float(p[l]));
    } else if (kind == 0) {
      const uint32_t* p = S.wimg[mode * GAIT_MODE_WORDS + r];
      for (int l = 0; l < GAIT_ENVS; ++l) x += (double)p[l];
    }
    part_out[(size_t)blockIdx.x * KBJ_GAIT_SIZE + tid] = x;
  }
}

}  // namespace
}  // namespace kbj
