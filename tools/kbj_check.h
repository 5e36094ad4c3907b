// What the kernel checks under tools/ share (gemm_check, reduce_check, lstm_check, head_check, update_check): error exit, hashes and fill values, rounding constants,
// the documented-order sums, the guarded device memory and the tally with its closing lines. Each tool is ONE translation unit that
// includes this header once; value families, bounds, case tables and `case` lines are the tool's own.
//
// GUARD SCHEME. All device memory of a tool comes from one Arena: a single allocation with 4 MB of unused slack at both ends, NaN
// (bytes 0xFF, in fp32 and fp64 alike) everywhere at the start and again, after every reset(), wherever a case had data. A kernel that
// strays by a whole tile therefore still reads mapped memory, reads NaN there, and fails a check instead of faulting. A one-dimensional
// array is uploaded as a window (put / get) with GUARD = 64 words in front and behind: NaN around an input, so that a read outside
// poisons the result, and the bit pattern 0xDEADBEEF (fp64: twice) around an output, which must be unchanged after the launch - a changed
// guard word is a stray store. Padding inside a window (columns between N and a leading dimension) is the tool's to fill and to compare.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <cmath>
#include <limits>
#include <algorithm>
#include <vector>
#include <string>
#include "kbj_ctx.h"

thread_local kbj_ctx* kbj_prof_ctx = nullptr;   // the library's globals that the launch helpers of the kernel headers refer to
thread_local std::string kbj_global_error;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); fflush(stdout); exit(2); } } while (0)

// ---- hashes of (array, row, column) and what is made of them ----
static inline uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
static inline uint32_t hash3(uint32_t tag, uint32_t r, uint32_t c) { return mix(mix(mix(tag) + r * 0x9E3779B9u) + c * 0x85EBCA6Bu + 1u); }
static inline int pick(int row, int salt, int n) { return (int)(mix((uint32_t)row * 31u + (uint32_t)salt * 0x632BE5ABu + 7u) % (uint32_t)n); }
static inline float val_real(uint32_t h) { return (float)((int)(h >> 8) - (1 << 23)) * (1.0f / (float)(1 << 23)); }   // uniform(-1, 1) on a 24-bit grid

// ---- fill values (float or double) and the bit-for-bit comparison ----
template <class T> static T pattern() { const uint64_t b = 0xDEADBEEFDEADBEEFull; T t; memcpy(&t, &b, sizeof(T)); return t; }
template <class T> static T qnan() { return std::numeric_limits<T>::quiet_NaN(); }
template <class T> static bool same_bits(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }
static const float PATTERN = pattern<float>(), QNAN = qnan<float>();

// ---- fp32 rounding (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1): n roundings in ANY order, error <= gamma_n sum |terms| ----
static const double U = std::ldexp(1.0, -24);
static inline double gamma_n(double n) { return n * U / (1.0 - n * U); }

// ---- a sum in the documented order (chain), and in the order that must NOT pass for it (balanced tree); elements `stride` apart ----
template <class T> static T chain(const T* v, size_t n, size_t stride) { T s = 0; for (size_t i = 0; i < n; ++i) s += v[i * stride]; return s; }
template <class T> static T tree(const T* v, size_t n, size_t stride) {
  if (n == 0) return 0;
  if (n == 1) return v[0];
  const size_t h = n / 2;
  return tree(v, h, stride) + tree(v + h * stride, n - h, stride);
}

// ---- guarded device memory (GUARD SCHEME above) ----
constexpr int GUARD = 64;
template <class T> struct Win { T* d = nullptr; size_t n = 0; };
struct Arena {
  static constexpr size_t SLACK = (size_t)4 << 20;
  const size_t cap; char* base = nullptr; size_t used = SLACK, high = SLACK;
  explicit Arena(size_t capacity) : cap(capacity) {}
  void init() { CK(hipMalloc(reinterpret_cast<void**>(&base), cap)); CK(hipMemset(base, 0xFF, cap)); }
  void reset() { if (high > SLACK) CK(hipMemset(base + SLACK, 0xFF, high - SLACK)); used = high = SLACK; }   // NaN again up to the high-water mark
  void* take(size_t bytes) {   // 256-byte aligned
    used = (used + 255) / 256 * 256;
    if (used + bytes > cap - SLACK) { printf("arena too small\n"); exit(2); }
    void* p = base + used; used += bytes; high = used; return p;
  }
  // uploads `v` between guards: NaN around an input, the pattern around an output
  template <class T> Win<T> put(const std::vector<T>& v, bool output) {
    std::vector<T> img(v.size() + 2 * GUARD, output ? pattern<T>() : qnan<T>());
    std::copy(v.begin(), v.end(), img.begin() + GUARD);
    Win<T> w; w.n = v.size(); w.d = reinterpret_cast<T*>(take(img.size() * sizeof(T))) + GUARD;
    CK(hipMemcpy(w.d - GUARD, img.data(), img.size() * sizeof(T), hipMemcpyHostToDevice));
    return w;
  }
  // copies an output window back into `v`; false: a guard word changed
  template <class T> bool get(const Win<T>& w, std::vector<T>& v) {
    std::vector<T> img(w.n + 2 * GUARD);
    CK(hipMemcpy(img.data(), w.d - GUARD, img.size() * sizeof(T), hipMemcpyDeviceToHost));
    bool ok = true;
    for (int i = 0; i < GUARD; ++i) ok = ok && same_bits(img[i], pattern<T>()) && same_bits(img[GUARD + w.n + i], pattern<T>());
    v.assign(img.begin() + GUARD, img.begin() + GUARD + w.n);
    return ok;
  }
};

// ---- the tally: each tool prints its own `case ...` lines and counts them here; finish() closes the report ----
struct Tally {
  bool plan_mode = false; int cases = 0, failures = 0;
  void args(int argc, char** argv) { plan_mode = argc > 1 && std::string(argv[1]) == "--plan"; }
  void count(bool ok) { ++cases; if (!ok) ++failures; }
  int finish(const char* name) {   // the `cases N` line, the closing banner; returns the exit status
    printf("cases %d\n", cases);
    if (failures) { printf("%s CHECK FAILED: %d of %d cases\n", name, failures, cases); return 1; }
    printf(plan_mode ? "%s CHECK PLAN OK\n" : "%s CHECK PASSED\n", name);
    return 0;
  }
};
static Tally tally;
