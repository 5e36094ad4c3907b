// kbj_window_scan.h — the two shapes the event statistics share (kbj_push_recovery.h, kbj_step_response.h): the ordered walk of one
// scheduled window per env, and the staging of the resulting records for their ordered statistics per group of envs. Included by kbj_traj_stats.hip.
//
// window_walk. One env per lane, one wavefront per workgroup of 64 consecutive envs. An env's window is the rows [first, end): `hold` rows
// in front of the scheduled row s, then the rows from s to the end of the window or of the trajectory. The walk is ordered in t, the fetches
// are not: a chunk of TC rows is loaded into registers while the chunk before it is scanned (two register images, swapped by unrolling the
// chunk loop twice), so a chunk costs one memory round trip that flies under the scan of its predecessor. Only the rows any lane of the
// wavefront needs are touched: [min first, max end), chunks aligned to multiples of TC, and the walk ends as soon as every lane has its
// outcome. What a row holds, how it is fetched and what the rule makes of it are the caller's.
// The group reduce (push_recovery_reduce_kernel, step_reduce_kernel). One workgroup, thread g owns group g and walks ALL envs in env order -
// the record rows are staged through LDS 256 envs at a time (group_stage_round: coalesced loads; every thread then reads the same LDS word:
// a broadcast) - adding in doubles. A fixed order without atomics: the same inputs give the same bytes on every call. (ordered_reduce_kernel
// folds ranges of partials and then the ranges: not an env-order sum.) A thread g >= G owns no group; an env whose group is outside [0, G)
// is in none.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include "kbj.h"

namespace kbj {
namespace {

constexpr int WINDOW_ENVS = 64;            // envs per workgroup of a walk = lanes of its one wavefront
constexpr int GROUP_REDUCE_THREADS = 256;  // the group reduce: one thread per group, and the envs staged per round
static_assert(GROUP_REDUCE_THREADS == 256, "the G range kbj.h documents for kbj_push_recovery and kbj_step_response: [1, 256]");

// one lane's window. `tail` is the number of rows from s to the end of the window, in 64 bits: the schedule is the caller's, no 32-bit
// overflow whatever it holds.
// end >= s whenever `scan` holds: scan gives s < T, and with tail >= 0 (the entry points refuse a negative window, a push length below 0
// counts as 0) end64 = s + tail >= s in 64 bits, so end = min(end64, T) >= s. Without `scan` first = end = 0: the window is empty.
struct Window {
  bool scan;          // the env is live and its rows [s - hold, s] exist: hold <= s < T
  int s, first, end;  // the scheduled row; the rows this lane reads: [first, end)
  long long end64;    // where the window would end in a trajectory long enough: end64 > T says the trajectory cut it
  __device__ Window(bool live, int s_, int hold, long long tail, int T) : scan(live && s_ >= hold && s_ < T), s(s_), end64((long long)s_ + tail) {
    first = scan ? s - hold : 0;
    end = scan ? (int)(end64 < (long long)T ? end64 : (long long)T) : 0;
  }
};

// walks the rows [first, end) of every lane's window in order. fetch(Row&, t) loads row t of this lane's env, rule(const Row&, t) applies
// it and sets `decided` once the lane needs no further row. Both are called only for first <= t < end, so 0 <= t < T and env < N, and the
// rule only while the lane is undecided. The caller starts `decided` at true for a lane without a window (!w.scan).
template <int TC, class Row, class Fetch, class Rule>
__device__ inline void window_walk(const Window& w, bool& decided, Fetch fetch, Rule rule) {
  // the rows this wavefront touches: [lo, hi)
  int lo = w.scan ? w.first : INT_MAX, hi = w.end;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
  if (hi <= lo) return;

  Row a[TC], b[TC];
  auto fetch_chunk = [&](Row (&r)[TC], int c) {              // chunk c = rows [c TC, (c + 1) TC); a lane loads what it will read
#pragma unroll
    for (int k = 0; k < TC; ++k) {
      const int t = c * TC + k;
      if (w.scan && t >= w.first && t < w.end) fetch(r[k], t);
    }
  };
  auto scan_chunk = [&](const Row (&r)[TC], int c) {
#pragma unroll
    for (int k = 0; k < TC; ++k) {
      const int t = c * TC + k;
      if (decided || t < w.first || t >= w.end) continue;
      rule(r[k], t);
    }
  };
  const int c0 = lo / TC, c1 = (hi - 1) / TC;                // first and last chunk
  fetch_chunk(a, c0);
  for (int c = c0; c <= c1; c += 2) {                        // every condition here is uniform over the wavefront
    if (__all(decided)) break;                               // nobody reads another row
    if (c + 1 <= c1) fetch_chunk(b, c + 1);
    scan_chunk(a, c);
    if (c + 1 > c1 || __all(decided)) break;
    if (c + 2 <= c1) fetch_chunk(a, c + 2);
    scan_chunk(b, c + 1);
  }
}

// One round of a group reduce: the records of the envs [n0, n0 + nb) and their groups into LDS (W floats per record, a multiple of 4). The
// barrier in front: every thread has read the round before. group == null: every env is in group 0.
// Only the staging is shared. A group_reduce_kernel<Group> with the accumulators in a struct and add(row) / store(out) as its members was
// built and dropped: add() is simplified on its own before it is inlined, where the accumulators are memory behind `this`, and there the
// compiler folds look-alike branches (steps to recovery / steps to the fall, overshoot / deviation) into one body with a selected member
// offset. No later pass can take that apart: 56 and 72 bytes of scratch per lane, where the kernels with local accumulators have none.
template <int W>
__device__ inline void group_stage_round(float (&row)[GROUP_REDUCE_THREADS][W], int (&grp)[GROUP_REDUCE_THREADS], const float* __restrict__ rec,
                                         const int32_t* __restrict__ group, int n0, int nb) {
  static_assert(W % 4 == 0, "a record row is staged as 16-byte pieces");
  __syncthreads();                                            // the round before has been read
  for (int i = threadIdx.x; i < nb * (W / 4); i += GROUP_REDUCE_THREADS)
    reinterpret_cast<float4*>(&row[0][0])[i] = reinterpret_cast<const float4*>(rec + (size_t)n0 * W)[i];
  if (threadIdx.x < nb) grp[threadIdx.x] = group ? group[n0 + threadIdx.x] : 0;
  __syncthreads();
}

}  // namespace
}  // namespace kbj
