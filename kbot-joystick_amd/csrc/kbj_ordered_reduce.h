// kbj_ordered_reduce.h — the second stage of the trajectory scans that leave workgroup partials (kbj_episode_stats.h, kbj_tracking_stats.h,
// kbj_gait_stats.h): the partials of a scan, [nblocks][SIZE] doubles, combined slot by slot in block order by ONE workgroup. Doubles, a fixed
// order, no atomics: the same partials give the same bytes on every call. Included by kbj_traj_stats.hip. (The event statistics,
// kbj_push_recovery.h and kbj_step_response.h, leave a record per env and have a second stage of their own: kbj_window_scan.h.)
// A vector wider than one workgroup (kbj_actuator_stats.h) takes ordered_reduce_wide_kernel, one workgroup per 256 slots.
//
// `Slots` says what a statistics vector is made of:
//   static constexpr int SIZE;                              slots per vector, a divisor of ORDERED_REDUCE_THREADS (wide: a multiple)
//   static __device__ double identity(int j);               the value of slot j over nothing
//   static __device__ double combine(int j, double a, double b);   slot j of the union, `a` being the earlier part
// The scans use the same combine for their lanes, in lane order.
#pragma once
#include <hip/hip_runtime.h>

namespace kbj {
namespace {

constexpr int ORDERED_REDUCE_THREADS = 256;

// the slots of a vector of counts and sums, but for some maxima of non-negative quantities: the identity of every slot is 0. `Derived`
// supplies SIZE and is_max(j). A loop over one slot hoists is_max(j) and calls combine_as
template <class Derived> struct SumMaxSlots {
  static __device__ inline double identity(int) { return 0.0; }
  static __device__ inline double combine_as(bool is_max, double a, double b) { return is_max ? (b > a ? b : a) : a + b; }   // is_max(j), hoisted by the caller
  static __device__ inline double combine(int j, double a, double b) { return combine_as(Derived::is_max(j), a, b); }
};

// one workgroup of ORDERED_REDUCE_THREADS: thread (r, j) folds slot j over the r-th of R = THREADS / SIZE contiguous ranges of blocks, in
// block order; then the threads of range 0 fold the ranges 1 .. R - 1 onto theirs, in order -> stats [SIZE]
template <class Slots>
__global__ __launch_bounds__(ORDERED_REDUCE_THREADS) void ordered_reduce_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ stats) {
  constexpr int SIZE = Slots::SIZE, R = ORDERED_REDUCE_THREADS / SIZE;
  static_assert(ORDERED_REDUCE_THREADS % SIZE == 0 && R >= 1, "every thread owns one (range, slot) of the LDS array");
  __shared__ double s[R][SIZE];
  const int j = threadIdx.x % SIZE, r = threadIdx.x / SIZE;
  const int per = (nblocks + R - 1) / R, b1 = min(nblocks, (r + 1) * per);
  double v = Slots::identity(j);
  for (int b = r * per; b < b1; ++b) v = Slots::combine(j, v, part[(size_t)b * SIZE + j]);
  s[r][j] = v;
  __syncthreads();
  if (r == 0) {
    for (int q = 1; q < R; ++q) v = Slots::combine(j, v, s[q][j]);
    stats[j] = v;
  }
}

// the same second stage for a vector wider than one workgroup (kbj_actuator_stats.h): SIZE a multiple of ORDERED_REDUCE_THREADS, a grid of
// SIZE / ORDERED_REDUCE_THREADS workgroups, thread j of workgroup g folds slot 256 g + j over all blocks in block order -> stats [SIZE]
template <class Slots>
__global__ __launch_bounds__(ORDERED_REDUCE_THREADS) void ordered_reduce_wide_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ stats) {
  constexpr int SIZE = Slots::SIZE;
  static_assert(SIZE % ORDERED_REDUCE_THREADS == 0 && SIZE >= ORDERED_REDUCE_THREADS, "every thread of the grid owns one slot");
  const int j = blockIdx.x * ORDERED_REDUCE_THREADS + threadIdx.x;
  if (j >= SIZE) return;
  constexpr int AHEAD = 8;      // loads in flight per thread: the fold is a chain of dependent adds, the loads are not
  double v = Slots::identity(j);
  int b = 0;
  for (; b + AHEAD <= nblocks; b += AHEAD) {
    double x[AHEAD];
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) x[k] = part[(size_t)(b + k) * SIZE + j];
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) v = Slots::combine(j, v, x[k]);
  }
  for (; b < nblocks; ++b) v = Slots::combine(j, v, part[(size_t)b * SIZE + j]);
  stats[j] = v;
}

}  // namespace
}  // namespace kbj
