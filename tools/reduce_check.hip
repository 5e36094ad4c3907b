// Bit-for-bit check of the ordered second stages of the deterministic update (kbj_config.deterministic) on synthetic partials:
//   reduce_rows_kernel, reduce_double_kernel (kbj_nn_kernels.h) and splitk_reduce_kernel (kbj_gemm.h), each through the launch helper the
//   call sites of kbj_nn.hip use.
//   make -C tools reduce_check && tools/reduce_check        (GPU; ends with REDUCE CHECK PASSED or a non-zero exit status)
//   tools/reduce_check --plan                               (no device: the same case table, proves that every input tells a tree from the chain)
//
// WHAT IS CHECKED. Every kernel's documented result is a chain: s = 0; s += partial 0; s += partial 1; ...; out += s, in the partials'
// index order, in the partials' own precision. The reference is that chain on the host, compared BIT FOR BIT with what the kernel leaves in
// `out`. How the kernels fetch the partials (batched loads, LDS staging) is free; the order of the additions is not.
//
// INPUTS for which the order matters: partial = sign * 2^e * (1 + 46-bit fraction, rounded to the kernel's precision) with e uniform in [-20, 20] (hash of kernel, case,
// partial index and column), a non-zero initial `out` of the same family. Before a case is launched the host also forms the PAIRWISE
// (balanced tree) sum of the same partials and requires that it differs from the chain in at least one output: a kernel that added in tree
// order - or in any order that a tree and a chain cannot be told apart by - could not pass by accident. The seed of a case is advanced until
// that holds (at most 64 times, else the case fails); with fewer than three partials a tree IS the chain, those cases say "order n/a".
//
// HARNESS (tools/kbj_check.h: the arena, the guarded window, the tally). Partials and split-K slabs are input windows: a partial read from
// outside the array, or from a split-K slice that the GEMM would not have written, poisons the sum if it is added. Outputs are output
// windows; the padding between N and ldc holds the bit pattern too and must be unchanged after the launch.
#include "kbj_check.h"
#include "kbj_gemm.h"
#include "kbj_nn_kernels.h"

using namespace kbj;

// sign * 2^e * (1 + fraction), e in [-20, 20]
static double value(uint32_t tag, uint32_t r, uint32_t c) {
  const uint32_t h = hash3(tag, r, c), h2 = mix(h ^ 0xA5A5A5A5u);
  const int e = (int)(h2 % 41u) - 20;
  const double m = 1.0 + (double)(h & 0x7FFFFFu) / 8388608.0 + (double)(mix(h2) >> 9) / 70368744177664.0;   // 46 fraction bits (fp32 cases round them)
  return std::ldexp((h >> 31) ? -m : m, e);
}

static Arena arena((size_t)16 << 20);
static void report(const char* kernel, const std::string& what, bool order_applies, bool ok, const char* why) {
  printf("case %-22s %-44s %s : %s%s\n", kernel, what.c_str(), order_applies ? "order matters" : "order n/a    ", ok ? (tally.plan_mode ? "planned" : "ok") : "FAIL ", ok ? "" : why);
  tally.count(ok);
}

// ---- column-wise second stages: reduce_rows (fp32, n columns) and reduce_double (fp64, w <= 64 columns) --------------------------------------
template <class T, class Launch>
static void column_case(const char* kernel, int nparts, int n, uint32_t id, Launch launch) {
  char what[96]; snprintf(what, sizeof what, "partials %d x %d", nparts, n);
  const bool order_applies = nparts >= 3;
  std::vector<T> part((size_t)nparts * n), out0(n), ref(n);
  uint32_t seed = id * 64u; bool found = !order_applies;
  for (int attempt = 0; attempt < 64; ++attempt, ++seed) {
    for (int p = 0; p < nparts; ++p) for (int c = 0; c < n; ++c) part[(size_t)p * n + c] = (T)value(seed * 2u, p, c);
    for (int c = 0; c < n; ++c) out0[c] = (T)value(seed * 2u + 1u, 0, c);
    bool differs = false;
    for (int c = 0; c < n; ++c) {
      T r = out0[c]; r += chain(&part[c], nparts, n); ref[c] = r;
      T t = out0[c]; t += tree(&part[c], nparts, n);
      differs = differs || !same_bits(r, t);
    }
    if (differs) found = true;
    if (found) break;
  }
  if (!found) { report(kernel, what, true, false, "no input found whose pairwise sum differs from the chain"); return; }
  if (tally.plan_mode) { report(kernel, what, order_applies, true, ""); return; }
  arena.reset();
  const Win<T> part_w = arena.put(part, false), out_w = arena.put(out0, true);
  launch(part_w.d, nparts, n, out_w.d);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<T> got;
  const bool guards = arena.get(out_w, got);
  bool exact = true;
  for (int c = 0; c < n; ++c) exact = exact && same_bits(got[c], ref[c]);
  report(kernel, what, order_applies, guards && exact, !guards ? "stray store (guard changed)" : "differs from the chain in slice order");
}

// ---- split-K second stage on hand-filled slabs -------------------------------------------------------------------------------------
static void splitk_case(int M, int N, int K, int sk, int n1, int ldc, int ldc2, uint32_t id) {
  const int per = ((K + sk - 1) / sk + GEMM_BK - 1) / GEMM_BK * GEMM_BK;
  int nks = 0; while (nks < sk && (long)nks * per < K) ++nks;          // the slices the GEMM writes
  char what[96]; snprintf(what, sizeof what, "%d x %d K=%d sk=%d (%d written)%s", M, N, K, sk, nks, n1 ? " paired" : "");
  const bool order_applies = nks >= 3;
  const size_t MN = (size_t)M * N;
  const int nA = n1 > 0 ? n1 : N, nB = N - nA;
  std::vector<float> slab((size_t)sk * MN), c0(MN), ref(MN);
  uint32_t seed = 0x40000000u + id * 64u; bool found = !order_applies;
  for (int attempt = 0; attempt < 64; ++attempt, ++seed) {
    for (int ks = 0; ks < sk; ++ks) for (size_t i = 0; i < MN; ++i) slab[ks * MN + i] = ks < nks ? (float)value(seed * 2u, ks, (uint32_t)i) : QNAN;
    bool differs = false;
    for (size_t i = 0; i < MN; ++i) {
      c0[i] = (float)value(seed * 2u + 1u, 0, (uint32_t)i);
      float r = c0[i]; r += chain(&slab[i], nks, MN); ref[i] = r;
      float t = c0[i]; t += tree(&slab[i], nks, MN);
      differs = differs || !same_bits(r, t);
    }
    if (differs) found = true;
    if (found) break;
  }
  if (!found) { report("splitk_reduce", what, true, false, "no input found whose pairwise sum differs from the chain"); return; }
  if (tally.plan_mode) { report("splitk_reduce", what, order_applies, true, ""); return; }
  // C [M][ldc] (columns < nA), C2 [M][ldc2] (the second problem's nB columns): pattern in the padding
  std::vector<float> cimg((size_t)M * ldc, PATTERN), c2img((size_t)M * ldc2 * (nB > 0), PATTERN);
  for (int m = 0; m < M; ++m) for (int n = 0; n < N; ++n) {
    if (n < nA) cimg[(size_t)m * ldc + n] = c0[(size_t)m * N + n];
    else c2img[(size_t)m * ldc2 + (n - nA)] = c0[(size_t)m * N + n];
  }
  arena.reset();
  const Win<float> slab_w = arena.put(slab, false), c_w = arena.put(cimg, true), c2_w = arena.put(c2img, true);
  GemmArgs g{nullptr, nullptr, c_w.d, nullptr, M, N, K, 0, 0, ldc, 1, sk, nullptr};
  if (nB) { g.C2 = c2_w.d; g.n1 = n1; g.ldc2 = ldc2; }
  g.skws = slab_w.d;
  splitk_reduce_launch(0, g, sk);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<float> got, got2;
  bool guards = arena.get(c_w, got), exact = true;
  guards = arena.get(c2_w, got2) && guards;
  auto scan = [&](const std::vector<float>& gimg, const std::vector<float>& img, int ld, int cols, int col0) {
    for (size_t i = 0; i < gimg.size(); ++i) {
      const size_t m = i / ld, n = i % ld;
      if ((int)n >= cols) guards = guards && same_bits(gimg[i], img[i]);
      else exact = exact && same_bits(gimg[i], ref[m * N + col0 + n]);
    }
  };
  scan(got, cimg, ldc, nA, 0);
  if (nB) scan(got2, c2img, ldc2, nB, nA);
  report("splitk_reduce", what, order_applies, guards && exact, !guards ? "stray store (guard or padding changed)" : "differs from the chain in slice order");
}

int main(int argc, char** argv) {
  tally.args(argc, argv);
  if (!tally.plan_mode) arena.init();
  // reduce_rows: one and several column blocks, ragged widths, one to 512 partial rows (the call sites: 16 / 32 row groups x H or 4H columns,
  // 512 rows x 1 / 40 columns)
  static const int RR[7][2] = {{1, 1}, {16, 256}, {32, 1024}, {33, 257}, {512, 1}, {512, 40}, {511, 65}};
  for (int i = 0; i < 7; ++i)
    column_case<float>("reduce_rows", RR[i][0], RR[i][1], 100u + i, [](const float* p, int np, int n, float* o) { reduce_rows_launch(0, p, np, n, o); });
  // reduce_double: the advantage statistics (32 x 2), the gradient norm (512 x 1), ragged and full-width forms
  static const int RD[5][2] = {{1, 1}, {32, 2}, {512, 1}, {513, 3}, {7, 64}};
  for (int i = 0; i < 5; ++i)
    column_case<double>("reduce_double", RD[i][0], RD[i][1], 200u + i, [](const double* p, int nb, int w, double* o) { reduce_double_launch(0, p, nb, w, o); });
  // split-K: K = 96 sk so that every slice is written (per = 96)
  static const int SMN[2][2] = {{70, 130}, {128, 256}};
  static const int SK[2] = {2, 24};
  uint32_t id = 0;
  for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) splitk_case(SMN[a][0], SMN[a][1], 96 * SK[b], SK[b], 0, SMN[a][1] + 12, 0, id++);
  splitk_case(70, 130, 100, 24, 0, 130, 0, id++);        // per = 32: slices 0 .. 3 written, 20 trailing slices hold NaN and must be skipped
  splitk_case(70, 130, 33, 7, 0, 133, 0, id++);          // per = 32: two written (the last one k), five empty
  splitk_case(70, 130, 96 * 24, 24, 64, 72, 67, id++);   // paired: columns >= n1 = 64 go to C2 with its own, unaligned leading dimension
  splitk_case(128, 256, 96 * 2, 2, 128, 128, 140, id++);
  return tally.finish("REDUCE");
}
