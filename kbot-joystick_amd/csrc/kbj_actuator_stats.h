// kbj_actuator_stats.h — what one trajectory asks of the motors (kbj_actuator_stats): per actuator torque against its level, joint speed,
// mechanical power, joint stops and the action rate, split by the command mode of the row (KBJ_AACC_*, KBJ_ACT_*, KBJ_AJNT_*, KBJ_AENV_*).
// Included by kbj_traj_stats.hip. The definitions are in kbj.h.
//
// Shape. The statistics are independent across actuators, so the scan runs one thread per (env, actuator): a workgroup of 320 threads owns
// 16 consecutive envs, thread e * 20 + u holds actuator u of env e. A row is fetched as coalesced 16-byte pieces, one chunk of 4 time steps
// ahead of the scan (the loads fly under the scan of the chunk before): per time step thread i loads piece i of the workgroup's aux rows
// (18 per env; the 12 that are read - QVEL, CTRL, CMD, DONE - through kbj_aux_stage.h), piece i of its qstate rows (20 per env; 1-6 hold the
// joint positions, 8-13 the joint speeds) and piece i of its action rows (5 per env): 29 pieces, 464 bytes per row. Staged in LDS the joint
// words are repacked to [env * 20 + u], so the scan reads them conflict-free.
// Per chunk: stage; 64 threads evaluate what a row has per env (mode, DONE, speed); all threads scan their actuator over the chunk's rows
// in ascending t and leave two bits per row (at the torque level, at a stop); one thread per env then folds the bits of its 20 actuators
// into the head slots, counts pairs and episodes. Three barriers per chunk.
// The accumulators are indexed by a run-time mode, so they are LDS images with the thread as the fastest index (as GaitShared's): per
// thread and mode five doubles (the real-valued sums) and seven words (three counts as uint32, four maxima as fp32 bits), 408 bytes per
// thread. That sets the envs per workgroup: 16 envs are 130,560 bytes of images, 27,904 of staged rows and 4,416 of head data - 162,880 of
// the 163,840 bytes of a CU. 8192 envs are 512 workgroups, two per CU one after the other. A command is held for seconds, so a thread keeps
// the current mode's twelve accumulators in registers and folds them into the mode's cells when the mode changes and behind the last row
// (twelve LDS read-modify-writes per thread and row otherwise; measured, that was 23 of 475 us at 8192 x 100 - the loads were the rest,
// see `fetch`); the sums associate by run of rows that share a mode, the runs in row order - still one fixed order. The env threads do
// the same with the head slots.
// Envs are combined in env order, in double, the workgroup partials in block order by ordered_reduce_wide_kernel over ActSlots: fixed
// order, no atomics - a call is bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "kbj_model.h"
#include "kbj_aux_stage.h"
#include "kbj_ordered_reduce.h"

namespace kbj {
namespace {

constexpr int ACT_ENVS = 16;                      // envs per workgroup
constexpr int ACT_TC = 4;                         // time steps per staging chunk
constexpr int ACT_THREADS = ACT_ENVS * KBJ_NU;    // 320: thread e * 20 + u
constexpr int ACT_Q_V4 = KBJ_QSTATE_SIZE / 4;     // 16-byte pieces of a qstate row
constexpr int ACT_A_V4 = KBJ_NU / 4;              // of an action row

// the kind of a joint slot: a 32-bit count (0), an fp32 maximum (1), a double sum (2)
__host__ __device__ constexpr int act_kind(int k) {
  return (k == KBJ_AJNT_TAU_MAX || k == KBJ_AJNT_VEL_MAX || k == KBJ_AJNT_POW_MAX || k == KBJ_AJNT_DACT_MAX) ? 1
       : (k == KBJ_AJNT_TAU_SQ || k == KBJ_AJNT_VEL_SQ || k == KBJ_AJNT_POW_ABS || k == KBJ_AJNT_POW_POS || k == KBJ_AJNT_DACT_SQ) ? 2 : 0;
}
// the index of joint slot k among the thread's words (kinds 0, 1) or among its doubles (kind 2)
__host__ __device__ constexpr int act_index(int k) {
  int n = 0;
  for (int j = 0; j < k; ++j) n += (act_kind(j) == 2) == (act_kind(k) == 2);
  return n;
}
constexpr int ACT_WORDS = act_index(KBJ_AJNT_DACT_MAX) + 1;   // 7 rows of the word image per mode
constexpr int ACT_DBLS = act_index(KBJ_AJNT_DACT_SQ) + 1;     // 5 rows of the double image per mode
constexpr int ACT_HEAD_WORDS = 4;                             // ROWS, PAIRS, ANY_TAU_ROWS, ANY_STOP_ROWS per env and mode; SPEED_SUM is a double
enum { ACT_HW_ROWS = 0, ACT_HW_PAIRS = 1, ACT_HW_ANY_TAU = 2, ACT_HW_ANY_STOP = 3 };

static_assert(ACT_WORDS == 7 && ACT_DBLS == 5 && ACT_WORDS + ACT_DBLS == KBJ_AJNT_SIZE, "joint block");
static_assert(KBJ_ACT_JOINT + KBJ_NU * KBJ_AJNT_SIZE <= KBJ_ACT_MODE_STRIDE && KBJ_CMODE_COUNT * KBJ_ACT_MODE_STRIDE == KBJ_ACT_EPISODES &&
              KBJ_ACT_EPISODES < KBJ_ACT_SIZE && KBJ_ACT_SIZE % ORDERED_REDUCE_THREADS == 0 && KBJ_ACT_ANY_STOP_ROWS < KBJ_ACT_JOINT, "actuator statistics layout");
static_assert(KBJ_AACC_PREV == 0 && KBJ_AACC_RUNNING == KBJ_NU && KBJ_AACC_SIZE == 24 && KBJ_AENV_SIZE == 12 && KBJ_NU % 4 == 0 && KBJ_QSTATE_SIZE % 4 == 0,
              "carry rows and per-env records are whole 16-byte pieces, RUNNING heads the last piece of a carry row");
static_assert(ACT_THREADS == ACT_ENVS * ACT_Q_V4 && ACT_THREADS >= ACT_ENVS * AUX_V4 && ACT_THREADS >= ACT_ENVS * ACT_A_V4 && ACT_THREADS >= ACT_TC * ACT_ENVS,
              "one piece of every source per thread and time step");

// the staged pieces of an aux row (kbj_aux_stage.h): those read are 0 (QVEL 0, 1) and 7-17 (CTRL, TOUCH, COMDIST, CMD, DONE)
struct ActMap {
  static constexpr int NPIECE = 12;
  static __device__ constexpr int piece(int p) { return p == 0 ? 0 : (p >= 7 && p <= 17) ? p - 6 : -1; }
};
using ActRow = StagedRow<ActMap>;
constexpr int ACT_LD = ActRow::LD;
static_assert(ActMap::piece((KBJ_AUX_QVEL + 1) / 4) == 0 && ActMap::piece(KBJ_AUX_CTRL / 4) == 1 && ActMap::piece((KBJ_AUX_CTRL + KBJ_NU - 1) / 4) >= 1 && ActMap::piece(KBJ_AUX_CMD / 4) >= 1 &&
              ActMap::piece(KBJ_AUX_DONE / 4) == ActMap::NPIECE - 1 && ActMap::piece(1) == -1 && ActMap::piece(6) == -1 && ACT_LD == 49 && KBJ_AUX_SIZE / 4 == 18, "staged pieces");
// the pieces of a qstate row that hold a joint position (columns QPOS + 7 ..) or a joint speed (QVEL + 6 ..)
__device__ constexpr bool act_q_piece(int p) {
  return (p >= (KBJ_QSTATE_QPOS + 7) / 4 && p <= (KBJ_QSTATE_QPOS + 7 + KBJ_NU - 1) / 4) || (p >= (KBJ_QSTATE_QVEL + 6) / 4 && p <= (KBJ_QSTATE_QVEL + 6 + KBJ_NU - 1) / 4);
}
static_assert(act_q_piece(1) && act_q_piece(6) && act_q_piece(8) && act_q_piece(13) && !act_q_piece(0) && !act_q_piece(7) && !act_q_piece(14), "qstate pieces 1-6 and 8-13");

struct ActStaged {                                   // one chunk's rows
  float aux[ACT_TC][ACT_ENVS * ACT_LD];              // [tt][env * ACT_LD + staged column]
  float q[ACT_TC][ACT_THREADS];                      // joint positions, [tt][env * 20 + u]
  float om[ACT_TC][ACT_THREADS];                     // joint speeds
  float act[ACT_TC][ACT_THREADS];                    // actions: the rows as they are in memory
};
struct ActFinal {                                    // the threads' totals of the call over all modes, for the per-env record
  double tot[4][ACT_THREADS];                        // TAU_SQ, POW_ABS, POW_POS, DACT_SQ
  float peak[ACT_THREADS];
};
struct ActShared {
  double dimg[KBJ_CMODE_COUNT * ACT_DBLS][ACT_THREADS];       // [mode * ACT_DBLS + row][thread]
  uint32_t wimg[KBJ_CMODE_COUNT * ACT_WORDS][ACT_THREADS];    // [mode * ACT_WORDS + row][thread]: counts as uint32, maxima as float bits
  double hspeed_sum[KBJ_CMODE_COUNT][ACT_ENVS];               // SPEED_SUM per env and mode
  double hspeed[ACT_TC][ACT_ENVS];                            // the chunk's rows per env: speed,
  uint32_t hflag[ACT_TC][ACT_ENVS];                           // mode | 8 where DONE == 0
  uint32_t himg[KBJ_CMODE_COUNT * ACT_HEAD_WORDS][ACT_ENVS];  // the head counts per env and mode
  uint32_t episodes[ACT_ENVS];
  union { ActStaged st; ActFinal fin; };                      // the totals are gathered where the rows were staged, behind the last chunk
  uint8_t bits[ACT_TC][ACT_THREADS];                          // per row and thread: 1 at the torque level, 2 at a stop
};
static_assert(ACT_THREADS % 4 == 0 && sizeof(ActFinal) <= sizeof(ActStaged) && offsetof(ActStaged, act) % 16 == 0 && sizeof(float[ACT_THREADS]) % 16 == 0, "the aliased totals fit; action rows are stored as 16-byte pieces");
static_assert(sizeof(ActShared) <= 160 * 1024, "one workgroup per CU");

// the slots of a KBJ_ACT vector (kbj_ordered_reduce.h): counts and sums, but for the four maxima of each joint block (each of a non-negative
// quantity)
struct ActSlots : SumMaxSlots<ActSlots> {
  static constexpr int SIZE = KBJ_ACT_SIZE;
  static __device__ inline bool is_max(int j) {
    if (j >= KBJ_ACT_EPISODES) return false;
    const int s = j % KBJ_ACT_MODE_STRIDE - KBJ_ACT_JOINT;
    return s >= 0 && s < KBJ_NU * KBJ_AJNT_SIZE && act_kind(s % KBJ_AJNT_SIZE) == 1;
  }
};

// grid = ceil(N / 16) workgroups of 320 threads; part_out [gridDim.x][KBJ_ACT_SIZE]; env_out [N][KBJ_AENV_SIZE] or null
__global__ __launch_bounds__(ACT_THREADS) void actuator_stats_kernel(const float* __restrict__ aux, const float* __restrict__ qstate, const float* __restrict__ action, int T, int N,
                                                                     const kbj_actuator_levels lv, float* __restrict__ acc, double* __restrict__ part_out, float* __restrict__ env_out) {
  __shared__ __align__(16) ActShared S;
  const int tid = threadIdx.x, e = tid / KBJ_NU, u = tid % KBJ_NU;
  const int e0 = blockIdx.x * ACT_ENVS, nb = min(ACT_ENVS, N - e0);
  const int nchunk = (T + ACT_TC - 1) / ACT_TC;
  const bool live = e < nb;                      // this thread's (env, actuator) exists
  const bool envt = tid < nb;                    // this thread also keeps env `tid`'s head slots

  for (int i = tid; i < KBJ_CMODE_COUNT * ACT_DBLS * ACT_THREADS; i += ACT_THREADS) (&S.dimg[0][0])[i] = 0.0;
  for (int i = tid; i < KBJ_CMODE_COUNT * ACT_WORDS * ACT_THREADS; i += ACT_THREADS) (&S.wimg[0][0])[i] = 0u;     // 0.0f as well
  for (int i = tid; i < KBJ_CMODE_COUNT * ACT_HEAD_WORDS * ACT_ENVS; i += ACT_THREADS) (&S.himg[0][0])[i] = 0u;
  for (int i = tid; i < KBJ_CMODE_COUNT * ACT_ENVS; i += ACT_THREADS) (&S.hspeed_sum[0][0])[i] = 0.0;
  if (tid < ACT_ENVS) S.episodes[tid] = 0u;

  // the thread's levels and carry, and its totals of this call over all modes
  float tau_level = 0.0f, vel_level = 0.0f, pos_lo = 0.0f, pos_hi = 0.0f;
#pragma unroll
  for (int j = 0; j < KBJ_NU; ++j)               // selects: a kernel argument indexed by u would be copied to scratch
    if (j == u) { tau_level = lv.tau_level[j]; vel_level = lv.vel_level[j]; pos_lo = lv.pos_lo[j]; pos_hi = lv.pos_hi[j]; }
  float* crow = acc + (size_t)(e0 + e) * KBJ_AACC_SIZE;
  float prev = 0.0f, running = 0.0f, peak = 0.0f;
  double tot_tau = 0.0, tot_pabs = 0.0, tot_ppos = 0.0, tot_dact = 0.0;
  if (live) { prev = crow[KBJ_AACC_PREV + u]; running = crow[KBJ_AACC_RUNNING]; }
  // the env thread's carry piece (RUNNING and the spare floats) and totals
  float4* ctail = reinterpret_cast<float4*>(acc + (size_t)(e0 + tid) * KBJ_AACC_SIZE + KBJ_AACC_RUNNING);
  float4 tail = make_float4(0, 0, 0, 0);
  uint32_t n_rows = 0, n_pairs = 0, n_any_tau = 0, n_any_stop = 0, n_episodes = 0;
  double speed_sum = 0.0;
  if (envt) tail = *ctail;

  // staging registers: piece `tid` of every source, for each time step of a chunk
  float4 va[ACT_TC], vq[ACT_TC], vc[ACT_TC];
  const bool ld_a = tid < nb * AUX_V4 && ActMap::piece(tid % AUX_V4) >= 0, ld_q = live && act_q_piece(tid % ACT_Q_V4), ld_c = tid < nb * ACT_A_V4;
  // Every thread loads on every time step, without a branch: a thread without a piece of a source takes the block's piece 0 again, a time
  // step beyond the last takes the last. Loads under per-thread conditions become one basic block each, and the compiler then waits for
  // the load before between them (it cannot see that the registers it reuses for the next address are free): twelve memory latencies
  // per chunk instead of one.
  const int ia = ld_a ? tid : 0, iq = ld_q ? tid : 0, ic = ld_c ? tid : 0;
  auto fetch = [&](int c) {
#pragma unroll
    for (int tt = 0; tt < ACT_TC; ++tt) {
      const size_t r0 = (size_t)min(c * ACT_TC + tt, T - 1) * N + e0;
      va[tt] = reinterpret_cast<const float4*>(aux + r0 * KBJ_AUX_SIZE)[ia];
      vq[tt] = reinterpret_cast<const float4*>(qstate + r0 * KBJ_QSTATE_SIZE)[iq];
      vc[tt] = reinterpret_cast<const float4*>(action + r0 * KBJ_NU)[ic];
    }
  };
  fetch(0);

  // the accumulators of the current mode live in registers and are folded into the mode's cells of the images when the mode changes (a
  // command is held for seconds) and behind the last row: sums associate by run of rows that share a mode, the runs in row order
  int cur = -1, hcur = -1;
  double rd[ACT_DBLS] = {0.0, 0.0, 0.0, 0.0, 0.0}, hspeed = 0.0;
  float rm[ACT_WORDS] = {0, 0, 0, 0, 0, 0, 0};         // indexed like the word image: the maxima's entries are used
  uint32_t rc[ACT_WORDS] = {0, 0, 0, 0, 0, 0, 0}, hc[ACT_HEAD_WORDS] = {0, 0, 0, 0};      // the counts' entries
  auto fold = [&]() {
    if (cur < 0) return;
    double (*D)[ACT_THREADS] = S.dimg + cur * ACT_DBLS;
    uint32_t (*W)[ACT_THREADS] = S.wimg + cur * ACT_WORDS;
#pragma unroll
    for (int k = 0; k < KBJ_AJNT_SIZE; ++k) {
      const int r = act_index(k);
      if (act_kind(k) == 2) { D[r][tid] += rd[r]; rd[r] = 0.0; }
      else if (act_kind(k) == 1) { W[r][tid] = __float_as_uint(fmaxf(__uint_as_float(W[r][tid]), rm[r])); rm[r] = 0.0f; }
      else { W[r][tid] += rc[r]; rc[r] = 0u; }
    }
  };
  auto hfold = [&]() {
    if (hcur < 0) return;
#pragma unroll
    for (int k = 0; k < ACT_HEAD_WORDS; ++k) { S.himg[hcur * ACT_HEAD_WORDS + k][tid] += hc[k]; hc[k] = 0u; }
    S.hspeed_sum[hcur][tid] += hspeed; hspeed = 0.0;
  };

  for (int c = 0; c < nchunk; ++c) {
    const int tc = min(ACT_TC, T - c * ACT_TC);
    // 1. the chunk's pieces into LDS
#pragma unroll
    for (int tt = 0; tt < ACT_TC; ++tt) {
      const bool row = tt < tc;
      if (row) stage_piece<ActMap>(S.st.aux[tt], va[tt], tid, nb * AUX_V4);
      if (row && ld_q) {
        const float w[4] = {vq[tt].x, vq[tt].y, vq[tt].z, vq[tt].w};
        const int col0 = 4 * (tid % ACT_Q_V4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int jq = col0 + k - (KBJ_QSTATE_QPOS + 7), jv = col0 + k - (KBJ_QSTATE_QVEL + 6);
          if (jq >= 0 && jq < KBJ_NU) S.st.q[tt][e * KBJ_NU + jq] = w[k];
          else if (jv >= 0 && jv < KBJ_NU) S.st.om[tt][e * KBJ_NU + jv] = w[k];
        }
      }
      if (row && ld_c) { float* d = S.st.act[tt] + 4 * tid; d[0] = vc[tt].x; d[1] = vc[tt].y; d[2] = vc[tt].z; d[3] = vc[tt].w; }
    }
    __syncthreads();
    if (c + 1 < nchunk) fetch(c + 1);            // the next chunk's loads fly under the scan
    // 2. what a row has per env: thread (tt, env)
    if (tid < ACT_TC * ACT_ENVS) {
      const int tt = tid / ACT_ENVS, en = tid % ACT_ENVS;
      if (tt < tc && en < nb) {
        const ActRow a{S.st.aux[tt] + en * ACT_LD};
        const double vx = (double)a[KBJ_AUX_QVEL], vy = (double)a[KBJ_AUX_QVEL + 1];
        S.hspeed[tt][en] = sqrt(vx * vx + vy * vy);
        S.hflag[tt][en] = (uint32_t)cmd_mode(a) | (a[KBJ_AUX_DONE] == 0.0f ? 8u : 0u);
      }
    }
    __syncthreads();
    // 3. the thread's actuator over the chunk's rows
    if (live) {
      const float* arow = S.st.aux[0] + e * ACT_LD + ActRow::col(KBJ_AUX_CTRL) + u;     // CTRL's 20 columns are staged side by side
      for (int s = 0; s < tc; ++s) {
        const uint32_t flags = S.hflag[s][e];
        const int mode = flags & 7;
        const float tau = arow[s * ACT_ENVS * ACT_LD], om = S.st.om[s][tid], q = S.st.q[s][tid], a = S.st.act[s][tid];
        const float P = __fmul_rn(tau, om), atau = fabsf(tau), aom = fabsf(om), aP = fabsf(P);
        const bool at_tau = atau >= tau_level, over = aom >= vel_level, at_stop = q <= pos_lo || q >= pos_hi;
        if (mode != cur) { fold(); cur = mode; }
        auto add = [&](int k, double x) { rd[act_index(k)] += x; };
        auto top = [&](int k, float x) { rm[act_index(k)] = fmaxf(rm[act_index(k)], x); };
        auto count = [&](int k, bool yes) { rc[act_index(k)] += yes ? 1u : 0u; };
        const double tau2 = (double)tau * (double)tau, ppos = (double)fmaxf(P, 0.0f);
        add(KBJ_AJNT_TAU_SQ, tau2); top(KBJ_AJNT_TAU_MAX, atau); count(KBJ_AJNT_TAU_ROWS, at_tau);
        add(KBJ_AJNT_VEL_SQ, (double)om * (double)om); top(KBJ_AJNT_VEL_MAX, aom); count(KBJ_AJNT_VEL_ROWS, over);
        add(KBJ_AJNT_POW_ABS, (double)aP); add(KBJ_AJNT_POW_POS, ppos); top(KBJ_AJNT_POW_MAX, aP); count(KBJ_AJNT_STOP_ROWS, at_stop);
        tot_tau += tau2; tot_pabs += (double)aP; tot_ppos += ppos;
        peak = fmaxf(peak, atau / tau_level);
        if (running != 0.0f) {
          const float d = a - prev;
          const double d2 = (double)d * (double)d;
          add(KBJ_AJNT_DACT_SQ, d2); top(KBJ_AJNT_DACT_MAX, fabsf(d));
          tot_dact += d2;
        }
        prev = a;
        running = (flags & 8u) ? 1.0f : 0.0f;
        S.bits[s][tid] = (uint8_t)((at_tau ? 1 : 0) | (at_stop ? 2 : 0));
      }
    }
    __syncthreads();
    // 4. the env's head slots: its 20 actuators' bits, pairs and episodes
    if (envt) {
      for (int s = 0; s < tc; ++s) {
        const uint32_t flags = S.hflag[s][tid];
        const int mode = flags & 7;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(S.bits[s]) + tid * (KBJ_NU / 4);     // the env's 20 bytes as five words
        uint32_t any = w[0] | w[1] | w[2] | w[3] | w[4];
        any = (any | any >> 8 | any >> 16 | any >> 24) & 3u;
        const double speed = S.hspeed[s][tid];
        const bool pair = tail.x != 0.0f;
        if (mode != hcur) { hfold(); hcur = mode; }
        hc[ACT_HW_ROWS] += 1u; hc[ACT_HW_ANY_TAU] += any & 1u; hc[ACT_HW_ANY_STOP] += (any >> 1) & 1u; hc[ACT_HW_PAIRS] += pair ? 1u : 0u;
        hspeed += speed;
        n_rows += 1; n_any_tau += any & 1u; n_any_stop += (any >> 1) & 1u; n_pairs += pair ? 1u : 0u; n_episodes += pair ? 0u : 1u;
        speed_sum += speed;
        tail.x = (flags & 8u) ? 1.0f : 0.0f;
      }
    }
    // the next chunk's staging writes S.st only, which step 4 does not read; S.hflag, S.hspeed and S.bits are written behind its barrier
  }
  if (live) fold();
  if (envt) hfold();
  __syncthreads();

  // the carry rows, and the threads' totals gathered per env
  if (live) {
    crow[KBJ_AACC_PREV + u] = prev;
    S.fin.tot[0][tid] = tot_tau; S.fin.tot[1][tid] = tot_pabs; S.fin.tot[2][tid] = tot_ppos; S.fin.tot[3][tid] = tot_dact;
    S.fin.peak[tid] = peak;
  }
  if (tid < ACT_ENVS) S.episodes[tid] = n_episodes;            // threads beyond the last env hold 0
  __syncthreads();
  if (envt) {
    *ctail = tail;
    if (env_out) {
      double sum[4] = {0.0, 0.0, 0.0, 0.0};
      float top = 0.0f;
      int top_u = -1;
      for (int j = 0; j < KBJ_NU; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[k] += S.fin.tot[k][tid * KBJ_NU + j];
        const float p = S.fin.peak[tid * KBJ_NU + j];
        if (top_u < 0 || p > top) { top = p; top_u = j; }
      }
      if (n_rows == 0) top_u = -1;
      float4* o = reinterpret_cast<float4*>(env_out + (size_t)(e0 + tid) * KBJ_AENV_SIZE);
      o[0] = make_float4((float)n_rows, (float)n_pairs, (float)speed_sum, (float)sum[0]);
      o[1] = make_float4((float)sum[1], (float)sum[2], (float)sum[3], (float)n_any_tau);
      o[2] = make_float4((float)n_any_stop, top, (float)top_u, 0.0f);
    }
  }
  // slot j of the partial: the envs in env order
  for (int j = tid; j < KBJ_ACT_SIZE; j += ACT_THREADS) {
    double x = 0.0;
    if (j == KBJ_ACT_EPISODES) {
      for (int l = 0; l < ACT_ENVS; ++l) x += (double)S.episodes[l];
    } else if (j < KBJ_ACT_EPISODES) {
      const int mode = j / KBJ_ACT_MODE_STRIDE, s = j % KBJ_ACT_MODE_STRIDE;
      if (s == KBJ_ACT_SPEED_SUM) {
        const double* p = S.hspeed_sum[mode];
        x = p[0];
        for (int l = 1; l < ACT_ENVS; ++l) x += p[l];
      } else if (s < KBJ_ACT_JOINT) {
        const int r = s == KBJ_ACT_ROWS ? ACT_HW_ROWS : s == KBJ_ACT_PAIRS ? ACT_HW_PAIRS : s == KBJ_ACT_ANY_TAU_ROWS ? ACT_HW_ANY_TAU : s == KBJ_ACT_ANY_STOP_ROWS ? ACT_HW_ANY_STOP : -1;
        if (r >= 0) {
          const uint32_t* p = S.himg[mode * ACT_HEAD_WORDS + r];
          for (int l = 0; l < ACT_ENVS; ++l) x += (double)p[l];
        }
      } else if (s < KBJ_ACT_JOINT + KBJ_NU * KBJ_AJNT_SIZE) {
        const int ju = (s - KBJ_ACT_JOINT) / KBJ_AJNT_SIZE, k = (s - KBJ_ACT_JOINT) % KBJ_AJNT_SIZE, kind = act_kind(k), r = act_index(k);
        if (kind == 2) {
          const double* p = S.dimg[mode * ACT_DBLS + r] + ju;
          x = p[0];
          for (int l = 1; l < ACT_ENVS; ++l) x += p[l * KBJ_NU];
        } else {
          const uint32_t* p = S.wimg[mode * ACT_WORDS + r] + ju;
          for (int l = 0; l < ACT_ENVS; ++l) x = kind == 1 ? ActSlots::combine_as(true, x, (double)__uint_as_float(p[l * KBJ_NU])) : x + (double)p[l * KBJ_NU];
        }
      }
    }
    part_out[(size_t)blockIdx.x * KBJ_ACT_SIZE + j] = x;
  }
}

}  // namespace
}  // namespace kbj
