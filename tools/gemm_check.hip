// Correctness check of every form of the fp32 GEMM (kbj_gemm.h) against a plain double-precision reference at ragged shapes.
//   make -C tools gemm_check && tools/gemm_check            (GPU; ends with GEMM CHECK PASSED or a non-zero exit status)
//   tools/gemm_check --plan                                  (no device: enumerates the same table, proves the exactness preconditions)
// Every launch goes through gemm_launch<A_KC, B_KC>(stream, g, force_big), the entry point of the call sites in kbj_nn.hip, so the
// launcher's tile choice, the x3 eligibility (gemm_x3_form) and the split-K reduce launch are under test with the kernels. No timing.
//
// HARNESS (the same for every case; arena, fill values and tally: tools/kbj_check.h, which documents the guard scheme)
//  * Every operand and every output is a two-dimensional window (Mat) of a larger array from the arena: a guard band in front and behind
//    (8 rows + 256 floats) and, where the form allows ld > row length, padding behind every row. Operand guard and padding are NaN; in a
//    gathered A the stored rows that the index list does not name are NaN too. Output guard and padding hold the bit pattern and must be
//    bit-identical after the launch (rows beyond M and the columns between N and ldc included). The deterministic split-K slab starts as
//    NaN (a reduce that reads a slice nobody wrote shows) and its guard is checked like an output's.
//  * beta = 0 launches start from a NaN-filled C (the old value must not enter); beta = 1 and split-K launches start from known values that
//    the reference includes.
//  * No form of kbj_gemm.h reads padding by design: the buffer-load fast path is taken only for tiles whose rows and 32 k are all in range,
//    every other load is guarded element by element (GemmStage::load, X3Stage::load / load_gen). The check therefore poisons ALL padding.
//  * The reference is the triple loop ref(m, n) = C0 + bias[n] + sum_k A(m, k) B(n, k) in double over the LOGICAL operands (LA [M][K],
//    LB [N][K]); the stored arrays (layout, second k source, second problem along n, row gather) are scattered from the logical ones here,
//    independently of gemm_item. Every output element is compared.
//
// VALUE FAMILIES
//  (a) exact: A, B integers in [-31, 31], bias and C0 integers in [-1000, 1000], all hashes of (array, row, column) so that a transposed or
//      shifted fragment cannot cancel. Every product is an integer <= 961 and every partial sum in any order an integer of magnitude
//      <= 961 K + 2000 <= 459 436 < 2^24 (K <= 476): all exactly representable in fp32, so the fp32-MFMA chain, atomics in any order, the slab
//      reduce and the x3 kernel (|x| <= 31 has 5 significant bits: x = hi, mid = lo = 0, the three dropped products vanish) must return the
//      reference BIT FOR BIT.
//  (b) x3 piece coverage (launches that the x3 kernel serves, K <= 100): one operand takes x = +-(2^16 | 2^8 | 1 | 16 hash bits) < 2^17. Its 17
//      significant bits split into hi = bits 16..9, mid = bits 8..1 (bit 8 is set, so the remainder's top 8 bits end at bit 1), lo = bit 0 = 1:
//      all three pieces are non-zero. The other operand takes integers in [-2, 2] (hi only), so mid lo, lo mid, lo lo vanish again and every
//      piece product and partial sum is an integer of magnitude < 2^18 K + 2000, below 2^24 for K <= 63 whatever the values. For 64 <= K <= 100
//      the bound is met by the actual values (mean |x| ~ 1.5 * 2^16, mean |y| = 1.2): --plan verifies sum |a||b| + |bias| + |C0| < 2^24 for
//      every element of every (a) and (b) input, which is the proof that the bit-exact requirement is sound. Run both ways round.
//  (c) reals: A, B = sA, sB x uniform(-1, 1) (24-bit grid), bias and C0 = sA sB x uniform(-1, 1), with (sA, sB) cycling over {2^-20, 1, 2^20}^2
//      from case to case. Bound (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a sum of n + 1 terms formed by n
//      roundings in ANY order has error <= gamma_n sum |terms|, gamma_n = n u / (1 - n u), u = 2^-24): an output element is K products entered
//      by fused multiply-adds (one rounding each; the product itself is not rounded), one addition of the bias, one of C0 (beta) and, under
//      split-K, up to splitk additions that combine the slices (atomics or the reduce): n = K + splitk + 2 roundings, so
//          |c - ref| <= gamma_n (sum_k |a||b| + |bias| + |C0|),   n = K + splitk + 2   (splitk = 1 without split-K).
//      The x3 kernel: x = hi + mid + lo exactly, the pieces have the sign of x, so sum over the six kept piece products of |p| <= |a||b|, and
//      they enter the fp32 accumulator with at most one rounding each: 6 K roundings instead of K. The dropped products: |mid| < 2^-7 |x|,
//      |lo| < 2^-15 |x| (hi keeps 8 significant bits, mid the next 8 at most), so |mid lo| + |lo mid| + |lo lo| < (2 * 2^-22 + 2^-30) |a||b|
//      < 9 u |a||b|. gamma is superadditive, hence n_x3 = 6 K + splitk + 2 + 9.
//      The double reference's own error, gamma^(double)_(K+2) < (K + 2) 2^-52 of the same sum, is added to the bound (1e-9 of it).
//      The worst observed fraction of the bound is printed per form.
//
// CASES. Per call site of kbj_nn.hip, the M, N, K (or N2, (K, splitk), (k1, k2)) lists below are combined by a covering array: with
// P = the longest list, row (i, j), 0 <= i, j < P takes M[i % a], N[j % b], K[((i + j) % P) % c], which contains every pair of values of any two
// lists (for a fixed i, (i + j) % P runs over all residues). The remaining options (tile, bias, beta, atomics / slab, alignment, ldb2 / ldc2)
// are drawn per row from a hash of the row number. Every row runs twice: as the call site issues it, and with x3 = 1, where the tool asserts
// that gemm_x3_form picks what the comments of kbj_gemm.h promise (promised_x3 below restates them: plain, GEN or silent fallback).
// The widest launch is linear_bwd_weight2 with the folded layer's 475-column second problem (n1 + 475 columns: the table of call sites
// asks for that width); everything else stays within 257 x 257 x 476.
#include <map>
#include "kbj_check.h"
#include "kbj_gemm.h"

using namespace kbj;

enum Fam { EXACT = 0, PIECE_A = 1, PIECE_B = 2, REAL = 3 };
static float val_int(uint32_t h, int amp) { return (float)((int)(h % (uint32_t)(2 * amp + 1)) - amp); }
static float val_piece(uint32_t h) { const int v = 0x10000 | 0x101 | (int)(h & 0xFFFFu); return (h >> 31) ? -(float)v : (float)v; }

// ---- one stored array: a window [rows][len] with leading dimension ld inside a guarded host image / device allocation ----
struct Mat {
  int rows = 0, len = 0, ld = 0; size_t lead = 0; std::vector<float> h; float* d = nullptr; bool used = false;
  void shape(int rows_, int len_, int ld_, int misalign) {
    rows = rows_; len = len_; ld = ld_; used = true;
    const size_t guard = ((size_t)8 * ld + 256 + 3) / 4 * 4;    // a multiple of 4 floats: the window keeps the allocation's 16-byte alignment ...
    lead = guard + (size_t)misalign;                             // ... unless the case asks for a base offset by one float
    h.resize(lead + (size_t)rows * ld + guard);
  }
  void fill(float v) { std::fill(h.begin(), h.end(), v); }
  float& at(int r, int c) { return h[lead + (size_t)r * ld + c]; }
  float* dev() const { return d + lead; }
  bool inside(size_t i) const { if (i < lead) return false; const size_t o = i - lead; return o / ld < (size_t)rows && o % ld < (size_t)len; }
};

static Arena arena((size_t)64 << 20);
static void upload(Mat& m) { m.d = reinterpret_cast<float*>(arena.take(m.h.size() * 4)); CK(hipMemcpy(m.d, m.h.data(), m.h.size() * 4, hipMemcpyHostToDevice)); }

// ---- one case ----
struct Spec {
  const char* form = ""; bool akc = true, bkc = true;
  int M = 1, N = 1, K = 1;     // N: all columns of the launch (n1 + second problem's width)
  int fb = -1, bias = 0, beta = 0, sk = 1, slab = 0;
  int k1 = 0;                  // second k source: k >= k1 from A2 / B2
  int n1 = 0, ldb2 = 0, ldc2 = 0;
  int aB = 0, aN = 0;          // row gather of A
  int lda = 0, ldb = 0, ldc = 0;
  int misA = 0, misB = 0, misC = 0;   // base pointer offset by one float
  int id = 0;
};
static int pad4(int len) { return (len + 3) / 4 * 4 + 8; }   // padded, rows stay 16-byte aligned
static int odd4(int len) { return pad4(len) + 1; }           // padded, ld % 4 != 0

// what the comments of kbj_gemm.h promise for a launch with x3 = 1: 0 = silently the exact kernel, 1 = plain split kernel, 2 = GEN
//  - fallbacks: deterministic split-K slabs; M or N below 64; an operand whose base or leading dimension is not 16-byte aligned
//  - GEN (k-contiguous operands only, no split-K, no second problem): bias, a second k source (k1 a multiple of 32), a row gather,
//    K a multiple of 4 but not of 32; K % 4 != 0 falls back
//  - plain: both layouts on 128-wide tiles, the 64 x 64 form for k-contiguous operands only; split-K with atomics; the paired problem
//    when n1 falls on a tile boundary
static int promised_x3(const Spec& s, bool big) {
  if (s.slab || s.M < 64 || s.N < 64) return 0;
  if (s.misA || s.misB || (s.lda & 3) || (s.ldb & 3) || (s.n1 > 0 && ((s.ldb2 > 0 ? s.ldb2 : s.ldb) & 3))) return 0;
  const bool needs_gen = s.bias || s.k1 > 0 || s.aB > 0 || s.K % 32 != 0;
  if (needs_gen) return (s.akc && s.bkc && s.n1 == 0 && s.sk == 1 && s.K % 4 == 0 && s.k1 % 32 == 0) ? 2 : 0;
  if (!big && !(s.akc && s.bkc)) return 0;
  if (s.n1 > 0 && s.n1 % (big ? 128 : 64) != 0) return 0;
  return 1;
}

struct Logical {      // logical operands of one value family, and the reference
  std::vector<double> A, B, bias, C0, ref, sabs; double max_sabs = 0;
};
static void make_logical(const Spec& s, Fam fam, double sa, double sb, Logical& L) {
  const int M = s.M, N = s.N, K = s.K;
  const uint32_t tag = (uint32_t)s.id * 16u + (uint32_t)fam * 4u;
  L.A.resize((size_t)M * K); L.B.resize((size_t)N * K); L.bias.assign(N, 0.0); L.C0.assign((size_t)M * N, 0.0);
  for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) { const uint32_t h = hash3(tag, m, k);
    L.A[(size_t)m * K + k] = fam == EXACT ? val_int(h, 31) : fam == PIECE_A ? val_piece(h) : fam == PIECE_B ? val_int(h, 2) : (double)val_real(h) * sa; }
  for (int n = 0; n < N; ++n) for (int k = 0; k < K; ++k) { const uint32_t h = hash3(tag + 1, n, k);
    L.B[(size_t)n * K + k] = fam == EXACT ? val_int(h, 31) : fam == PIECE_B ? val_piece(h) : fam == PIECE_A ? val_int(h, 2) : (double)val_real(h) * sb; }
  const bool c0 = s.beta || s.sk > 1;
  if (s.bias) for (int n = 0; n < N; ++n) { const uint32_t h = hash3(tag + 2, 0, n); L.bias[n] = fam == REAL ? (double)val_real(h) * sa * sb : val_int(h, 1000); }
  if (c0) for (int m = 0; m < M; ++m) for (int n = 0; n < N; ++n) { const uint32_t h = hash3(tag + 3, m, n);
    L.C0[(size_t)m * N + n] = fam == REAL ? (double)val_real(h) * sa * sb : val_int(h, 1000); }
  L.ref.resize((size_t)M * N); L.sabs.resize((size_t)M * N); L.max_sabs = 0;
  for (int m = 0; m < M; ++m) for (int n = 0; n < N; ++n) {
    const double* a = &L.A[(size_t)m * K]; const double* b = &L.B[(size_t)n * K];
    double sum = 0, sab = 0;
    for (int k = 0; k < K; ++k) { const double p = a[k] * b[k]; sum += p; sab += std::fabs(p); }
    const double c = L.C0[(size_t)m * N + n];
    L.ref[(size_t)m * N + n] = sum + L.bias[n] + c;
    const double sa_ = sab + std::fabs(L.bias[n]) + std::fabs(c);
    L.sabs[(size_t)m * N + n] = sa_; L.max_sabs = std::max(L.max_sabs, sa_);
  }
}

struct Stored { Mat A, A2, B, B2, C, C2, bias, slab; std::vector<int> idx; int* idx_d = nullptr; };

// stored arrays of a case from its logical operands: layout, second k source, second problem along n, row gather (written out here)
static void make_stored(const Spec& s, const Logical& L, Stored& S) {
  const int M = s.M, N = s.N, K = s.K;
  const int nA = s.n1 > 0 ? s.n1 : N, nB = N - nA;        // columns of the first / second problem
  const int kA = s.k1 > 0 ? s.k1 : K, kB = K - kA;        // k of the first / second source
  const int ldb2 = s.ldb2 > 0 ? s.ldb2 : s.ldb, ldc2 = s.ldc2 > 0 ? s.ldc2 : s.ldc;
  S = Stored();
  // A
  if (s.akc) {
    if (s.aB > 0) {
      const int T = (M + s.aB - 1) / s.aB;
      std::vector<std::pair<uint32_t, int>> perm(s.aN);
      for (int i = 0; i < s.aN; ++i) perm[i] = {hash3((uint32_t)s.id * 16u + 9u, 0, i), i};
      std::sort(perm.begin(), perm.end());
      S.idx.resize(s.aB); for (int b = 0; b < s.aB; ++b) S.idx[b] = perm[b].second;      // a_B distinct env indices out of a_N, permuted
      S.A.shape(T * s.aN, K, s.lda, s.misA); S.A.fill(QNAN);
      for (int m = 0; m < M; ++m) { const int t = m / s.aB, b = m % s.aB; for (int k = 0; k < K; ++k) S.A.at(t * s.aN + S.idx[b], k) = (float)L.A[(size_t)m * K + k]; }
    } else {
      S.A.shape(M, kA, s.lda, s.misA); S.A.fill(QNAN);
      for (int m = 0; m < M; ++m) for (int k = 0; k < kA; ++k) S.A.at(m, k) = (float)L.A[(size_t)m * K + k];
      if (kB > 0) { S.A2.shape(M, kB, s.lda, 0); S.A2.fill(QNAN); for (int m = 0; m < M; ++m) for (int k = 0; k < kB; ++k) S.A2.at(m, k) = (float)L.A[(size_t)m * K + kA + k]; }
    }
  } else {
    S.A.shape(K, M, s.lda, s.misA); S.A.fill(QNAN);
    for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) S.A.at(k, m) = (float)L.A[(size_t)m * K + k];
  }
  // B (+ B2: the second k source of the same rows, or the second problem's rows)
  if (s.bkc) {
    S.B.shape(nA, kA, s.ldb, s.misB); S.B.fill(QNAN);
    for (int n = 0; n < nA; ++n) for (int k = 0; k < kA; ++k) S.B.at(n, k) = (float)L.B[(size_t)n * K + k];
    if (kB > 0) { S.B2.shape(nA, kB, s.ldb, 0); S.B2.fill(QNAN); for (int n = 0; n < nA; ++n) for (int k = 0; k < kB; ++k) S.B2.at(n, k) = (float)L.B[(size_t)n * K + kA + k]; }
    if (nB > 0) { S.B2.shape(nB, K, ldb2, 0); S.B2.fill(QNAN); for (int n = 0; n < nB; ++n) for (int k = 0; k < K; ++k) S.B2.at(n, k) = (float)L.B[(size_t)(nA + n) * K + k]; }
  } else {
    S.B.shape(K, nA, s.ldb, s.misB); S.B.fill(QNAN);
    for (int n = 0; n < nA; ++n) for (int k = 0; k < K; ++k) S.B.at(k, n) = (float)L.B[(size_t)n * K + k];
    if (nB > 0) { S.B2.shape(K, nB, ldb2, 0); S.B2.fill(QNAN); for (int n = 0; n < nB; ++n) for (int k = 0; k < K; ++k) S.B2.at(k, n) = (float)L.B[(size_t)(nA + n) * K + k]; }
  }
  // outputs: guard and padding = PATTERN; the logical window = C0 (beta / split-K) or NaN (beta = 0)
  const bool c0 = s.beta || s.sk > 1;
  S.C.shape(M, nA, s.ldc, s.misC); S.C.fill(PATTERN);
  for (int m = 0; m < M; ++m) for (int n = 0; n < nA; ++n) S.C.at(m, n) = c0 ? (float)L.C0[(size_t)m * N + n] : QNAN;
  if (nB > 0) { S.C2.shape(M, nB, ldc2, 0); S.C2.fill(PATTERN); for (int m = 0; m < M; ++m) for (int n = 0; n < nB; ++n) S.C2.at(m, n) = c0 ? (float)L.C0[(size_t)m * N + nA + n] : QNAN; }
  if (s.bias) { S.bias.shape(1, N, N, 0); S.bias.fill(QNAN); for (int n = 0; n < N; ++n) S.bias.at(0, n) = (float)L.bias[n]; }
  if (s.slab) { S.slab.shape(s.sk * M, N, N, 0); S.slab.fill(QNAN); }
}

static std::vector<float> got;

// copies an output back; false on a changed guard / padding word. The logical window lands in `got` at the Mat's own offsets.
static bool guards_intact(const Mat& m, bool keep) {
  std::vector<float> tmp; std::vector<float>& g = keep ? got : tmp;
  g.resize(m.h.size());
  CK(hipMemcpy(g.data(), m.d, g.size() * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < g.size(); ++i) if (!m.inside(i) && !same_bits(g[i], m.h[i])) return false;
  return true;
}

struct Outcome { bool ok = true; std::string why; double frac = 0; };
static void fail(Outcome& o, const char* why) { if (o.ok) { o.ok = false; o.why = why; } }

static int launcher_big(const Spec& s) {   // the tile the launcher will take (its rule, for gemm_x3_form's last argument)
  const long big_items = (long)((s.M + 127) / 128) * ((s.N + 127) / 128) * s.sk;
  return s.fb >= 0 ? s.fb != 0 : (big_items >= 192 && s.N > 64);
}

// one launch of one value family; x3form: what gemm_x3_form answered (decides the real family's n)
static Outcome run_one(const Spec& s, const Logical& L, Stored& S, Fam fam, int x3, int* x3form) {
  Outcome o;
  arena.reset();
  Mat* mats[8] = {&S.A, &S.A2, &S.B, &S.B2, &S.C, &S.C2, &S.bias, &S.slab};
  for (Mat* m : mats) if (m->used) upload(*m);
  if (!S.idx.empty()) { S.idx_d = reinterpret_cast<int*>(arena.take(S.idx.size() * 4)); CK(hipMemcpy(S.idx_d, S.idx.data(), S.idx.size() * 4, hipMemcpyHostToDevice)); }
  GemmArgs g{S.A.dev(), S.B.dev(), S.C.dev(), s.bias ? S.bias.dev() : nullptr, s.M, s.N, s.K, s.lda, s.ldb, s.ldc, s.beta, s.sk, nullptr};
  if (s.k1 > 0) { g.A2 = S.A2.dev(); g.B2 = S.B2.dev(); g.k1 = s.k1; }
  if (s.n1 > 0) { g.B2 = S.B2.dev(); g.C2 = S.C2.dev(); g.n1 = s.n1; g.ldb2 = s.ldb2; g.ldc2 = s.ldc2; }
  if (s.aB > 0) { g.a_idx = S.idx_d; g.a_B = s.aB; g.a_N = s.aN; }
  if (s.slab) g.skws = S.slab.dev();
  g.x3 = x3;
  *x3form = gemm_x3_form(g, s.akc, s.bkc, launcher_big(s));
  if (s.akc && s.bkc) gemm_launch<true, true>(0, g, s.fb);
  else if (s.akc) gemm_launch<true, false>(0, g, s.fb);
  else gemm_launch<false, false>(0, g, s.fb);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  const int nA = s.n1 > 0 ? s.n1 : s.N;
  const int sk = s.sk > 1 ? s.sk : 1;
  const double gam = gamma_n((*x3form ? 6.0 * s.K + 9.0 : (double)s.K) + sk + 2) + (s.K + 2) * std::ldexp(1.0, -52);
  for (int part = 0; part < (s.n1 > 0 ? 2 : 1); ++part) {
    const Mat& C = part ? S.C2 : S.C;
    if (!guards_intact(C, true)) fail(o, "stray store (guard or padding of C changed)");
    for (int m = 0; m < s.M; ++m) for (int n = 0; n < C.len; ++n) {
      const float c = got[C.lead + (size_t)m * C.ld + n];
      const size_t li = (size_t)m * s.N + (part ? nA : 0) + n;
      if (std::isnan(c)) { fail(o, "NaN in the result (read outside the logical operands, or C0 entered at beta = 0)"); continue; }
      if (fam == REAL) {
        const double bound = gam * L.sabs[li], err = std::fabs((double)c - L.ref[li]);
        if (bound > 0) o.frac = std::max(o.frac, err / bound);
        if (err > bound) fail(o, "outside the error bound");
      } else if (c != (float)L.ref[li]) fail(o, "not bit-exact");     // (float)ref is exact: an integer below 2^24; +0 == -0
    }
  }
  if (s.slab && !guards_intact(S.slab, false)) fail(o, "stray store (guard of the split-K slab changed)");
  return o;
}

struct FormStat { double frac = 0, frac_x3 = 0; int cases = 0, fails = 0; };
static std::map<std::string, FormStat> stats;
static std::vector<std::string> form_order;

static std::string describe(const Spec& s) {
  char b[512];
  int n = snprintf(b, sizeof b, "%-24s <%c,%c> fb=%2d M=%3d N=%3d K=%3d lda=%d ldb=%d ldc=%d", s.form, s.akc ? 'T' : 'F', s.bkc ? 'T' : 'F', s.fb, s.M, s.N, s.K, s.lda, s.ldb, s.ldc);
  auto add = [&](const char* f, int a = 0, int c = 0, int d = 0) { n += snprintf(b + n, sizeof b - n, f, a, c, d); };
  if (s.bias) add(" bias");
  add(" beta=%d", s.beta);
  if (s.sk > 1) add(s.slab ? " splitk=%d(slab)" : " splitk=%d(atomics)", s.sk);
  if (s.k1) add(" k1=%d", s.k1);
  if (s.n1) add(" n1=%d ldb2=%d ldc2=%d", s.n1, s.ldb2, s.ldc2);
  if (s.aB) add(" a_B=%d a_N=%d", s.aB, s.aN);
  if (s.misA) add(" A+1");
  if (s.misB) add(" B+1");
  if (s.misC) add(" C+1");
  return b;
}

static int next_id = 0;
// one row of the table: runs as the call site issues it and once more with x3 = 1
static void run_case(Spec s) {
  s.id = next_id++;
  if (stats.find(s.form) == stats.end()) form_order.push_back(s.form);
  FormStat& fs = stats[s.form];
  static const double scales[3] = {std::ldexp(1.0, -20), 1.0, std::ldexp(1.0, 20)};
  const double sa = scales[s.id % 3], sb = scales[(s.id / 3) % 3];
  const int promised = promised_x3(s, launcher_big(s));
  const bool pieces = promised != 0 && s.K <= 100;
  std::string res[2]; bool ok[2] = {true, true}; int form_seen[2] = {0, 0};
  const double lim = std::ldexp(1.0, 24);
  for (int fam = EXACT; fam <= REAL; ++fam) {
    if ((fam == PIECE_A || fam == PIECE_B) && !pieces) continue;
    Logical L; make_logical(s, (Fam)fam, sa, sb, L);
    const char* fname = fam == EXACT ? "exact" : fam == PIECE_A ? "pieceA" : fam == PIECE_B ? "pieceB" : "real";
    if (fam != REAL && !(L.max_sabs < lim)) {     // the exactness precondition of families (a) and (b), in units of the operands' ulp (1)
      for (int x3 = 0; x3 < 2; ++x3) { ok[x3] = false; res[x3] += std::string(" ") + fname + "=FAIL(precondition: sum |a||b| + |bias| + |C0| >= 2^24)"; }
      continue;
    }
    if (tally.plan_mode) continue;
    Stored S; make_stored(s, L, S);
    for (int x3 = 0; x3 < 2; ++x3) {
      if ((fam == PIECE_A || fam == PIECE_B) && !x3) continue;
      int form = 0;
      Outcome o = run_one(s, L, S, (Fam)fam, x3, &form);
      form_seen[x3] = form;
      char b[160];
      if (!o.ok) { ok[x3] = false; snprintf(b, sizeof b, " %s=FAIL(%s)", fname, o.why.c_str()); }
      else if (fam == REAL) { snprintf(b, sizeof b, " real=%.3f", o.frac); double& w = form ? fs.frac_x3 : fs.frac; w = std::max(w, o.frac); }
      else snprintf(b, sizeof b, " %s=ok", fname);
      res[x3] += b;
    }
  }
  for (int x3 = 0; x3 < 2; ++x3) {
    const int want = x3 ? promised : 0;
    if (!tally.plan_mode && form_seen[x3] != want) { ok[x3] = false; res[x3] += " x3form=FAIL(gemm_x3_form disagrees with the promise)"; }
    static const char* fn[3] = {"exact-kernel", "x3-plain", "x3-GEN"};
    printf("case %4d %s x3=%d->%s(TM=%d) :%s : %s\n", 2 * s.id + x3, describe(s).c_str(), x3, fn[want], launcher_big(s) ? 2 : 1, res[x3].c_str(),
           ok[x3] ? (tally.plan_mode ? "planned" : "ok") : "FAIL");
    tally.count(ok[x3]); ++fs.cases;
    if (!ok[x3]) ++fs.fails;
  }
}

template <class F> static void lattice(int a, int b, int c, F f) {
  const int P = std::max(a, std::max(b, c));
  for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) f(i % a, j % b, ((i + j) % P) % c, i * P + j);
}

static const int MN[10] = {1, 31, 40, 63, 64, 65, 127, 128, 129, 257};
static const int KS[12] = {1, 3, 4, 31, 32, 33, 63, 64, 65, 96, 100, 476};
// (K, splitk), per = ceil(K / splitk) rounded up to 32: {100,2} per 64: last slice partial; {30,2}, {32,2} per 32: slice 1 empty; {65,3} per 32: last
// slice one k; {476,7} per 96: slice 4 partial, 5 and 6 empty; {33,7} per 32: five trailing slices empty; {96,3}, {64,2}: all full (x3-eligible K);
// {1,3}: two empty; {63,2}; {4,7}: six empty; {476,3} per 160: last partial
static const int KSK[12][2] = {{100, 2}, {30, 2}, {65, 3}, {476, 7}, {33, 7}, {96, 3}, {64, 2}, {1, 3}, {63, 2}, {4, 7}, {476, 3}, {32, 2}};

// alignment options shared by the forms with free leading dimensions: 0-2 aligned, 3 A + 1 float, 4 B + 1 float, 5 lda % 4 != 0, 6 ldb % 4 != 0,
// 7 C + 1 float and ldc % 4 != 0. lenA / lenB / lenC: the stored row lengths
static void align_opts(Spec& s, int opt, int lenA, int lenB, int lenC) {
  s.lda = opt == 5 ? odd4(lenA) : pad4(lenA); s.ldb = opt == 6 ? odd4(lenB) : pad4(lenB); s.ldc = opt == 7 ? odd4(lenC) : pad4(lenC);
  s.misA = opt == 3; s.misB = opt == 4; s.misC = opt == 7;
}

// The second pass (elig) redraws every form from the sub-lists at which the x3 kernel is eligible (M, N >= 64, K a multiple of 4 or 32, aligned
// operands, atomics): the first pass alone meets those conditions together only a few times per form.
static const int MN6[6] = {64, 65, 127, 128, 129, 257};
static const int KE[6] = {32, 64, 96, 4, 100, 476};                                          // plain (K % 32 == 0) and GEN-only (K % 4 == 0)
static const int KSKE[6][2] = {{96, 3}, {64, 2}, {32, 2}, {96, 2}, {64, 7}, {96, 7}};        // K % 32 == 0; {32,2} one empty slice, {64,7} five, {96,7} four; {96,2} last partial

static void all_cases(bool elig) {
  const int nmn = elig ? 6 : 10, nk = elig ? 6 : 12;
  const int* mn = elig ? MN6 : MN; const int* ks = elig ? KE : KS; const int (*ksk)[2] = elig ? KSKE : KSK;
  // linear_fwd: y = x W^T + b
  lattice(nmn, nmn, nk, [&](int i, int j, int k, int r) {
    Spec s; s.form = "linear_fwd"; s.M = mn[i]; s.N = mn[j]; s.K = ks[k];
    static const int fb[3] = {-1, 0, 1}; s.fb = fb[pick(r, 1, 3)]; s.bias = pick(r, 2, 2); s.beta = pick(r, 3, 2);
    align_opts(s, elig ? 0 : pick(r, 4, 8), s.K, s.K, s.N); run_case(s); });
  // rollout gates: G = [x | h] [W_ih | W_hh]^T + b, lda = ldb = row length (k1 = H; the second length both a multiple of 32 and not)
  lattice(nmn, nmn, elig ? 6 : 10, [&](int i, int j, int k, int r) {
    static const int KK[10][2] = {{32, 32}, {64, 4}, {64, 100}, {96, 28}, {64, 64}, {32, 96}, {32, 33}, {32, 1}, {96, 31}, {64, 63}};   // the first six: K % 4 == 0
    Spec s; s.form = "rollout_gates"; s.M = mn[i]; s.N = mn[j]; s.k1 = KK[k][0]; s.K = KK[k][0] + KK[k][1];
    s.fb = pick(r, 1, 2) ? 0 : -1; s.bias = pick(r, 2, 4) != 0; s.beta = pick(r, 3, 4) == 0;
    s.lda = s.ldb = std::max(KK[k][0], KK[k][1]); s.ldc = pad4(s.N);
    const int o = elig ? 0 : pick(r, 4, 6); s.misA = o == 3; s.misB = o == 4; s.misC = o == 5; run_case(s); });
  // critic input projection: rows gathered through the minibatch's env indices; a_B below, equal to and above the 64-row tile (40 and 100 do not
  // divide / are not divided by it), a_N > a_B, tiles that span several time steps, interior tiles followed by a partial k tile (K = 476)
  lattice(nmn, nmn, nk, [&](int i, int j, int k, int r) {
    Spec s; s.form = "critic_input_projection"; s.M = mn[i]; s.N = mn[j]; s.K = ks[k];
    static const int fb[3] = {2, -1, 1}; s.fb = fb[pick(r, 1, 3)]; s.bias = pick(r, 2, 4) != 0; s.beta = 0;
    static const int aB[3] = {40, 64, 100}; s.aB = aB[pick(r, 3, 3)]; s.aN = s.aB + 10;
    int o = elig ? 0 : pick(r, 4, 8); if (o == 7) o = 0; align_opts(s, o, s.K, s.K, s.N); run_case(s); });
  // g2a: dW_ih0 += Z W_in with K = nin = 65 / 475 (not a multiple of 4), ldb = K (unaligned rows: guarded scalar path), A padded to ld_obs
  if (!elig) lattice(10, 10, 2, [&](int i, int j, int k, int r) {
    Spec s; s.form = "g2a"; s.M = MN[i]; s.N = MN[j]; s.K = k ? 475 : 65; s.fb = -1; s.beta = 1;
    s.lda = (s.K + 3) / 4 * 4; s.ldb = s.K; s.ldc = pick(r, 1, 2) ? s.N : pad4(s.N); run_case(s); });
  // linear_bwd_input: dx = dy W  (x3: the plain form on 128-wide tiles only)
  lattice(nmn, nmn, nk, [&](int i, int j, int k, int r) {
    Spec s; s.form = "linear_bwd_input"; s.bkc = false; s.M = mn[i]; s.N = mn[j]; s.K = ks[k];
    static const int fb[4] = {-1, 0, 1, 2}; s.fb = elig ? 1 + pick(r, 1, 2) : fb[pick(r, 1, 4)]; s.beta = pick(r, 3, 2);
    align_opts(s, elig ? 0 : pick(r, 4, 8), s.K, s.N, s.N); run_case(s); });
  // linear_bwd_weight: dW += dy^T x, split-K with atomics or the deterministic slab
  lattice(nmn, nmn, nk, [&](int i, int j, int k, int r) {
    Spec s; s.form = "linear_bwd_weight"; s.akc = s.bkc = false; s.M = mn[i]; s.N = mn[j]; s.K = ksk[k][0]; s.sk = ksk[k][1];
    s.fb = elig ? 1 : pick(r, 1, 2); s.beta = 1; s.slab = elig ? 0 : pick(r, 2, 2);
    align_opts(s, elig ? 0 : pick(r, 4, 8), s.M, s.N, s.N); run_case(s); });
  // linear_bwd_weight2 and the folded layer-0 launch: two weight gradients that share dy; the second problem's width ragged (65, 475),
  // ldb2 / ldc2 equal to (0), different from, and tight (unaligned for odd widths) against ldb / ldc
  lattice(nmn, elig ? 7 : 11, nk, [&](int i, int j, int k, int r) {
    static const int N2[11] = {64, 65, 127, 128, 129, 257, 475, 1, 31, 40, 63};
    Spec s; s.form = "linear_bwd_weight2"; s.akc = s.bkc = false; s.M = mn[i]; s.K = ksk[k][0]; s.sk = ksk[k][1];
    s.fb = elig ? 1 : pick(r, 1, 2); s.beta = 1; s.slab = elig ? 0 : pick(r, 2, 2);
    const int tile = s.fb ? 128 : 64; s.n1 = tile * (1 + (s.fb ? 0 : pick(r, 5, 2))); s.N = s.n1 + N2[j];
    const int mode = pick(r, 3, 3);
    align_opts(s, elig ? 0 : pick(r, 4, 8), s.M, mode == 0 ? std::max(s.n1, N2[j]) : s.n1, mode == 0 ? std::max(s.n1, N2[j]) : s.n1);
    if (mode == 1) { s.ldb2 = pad4(N2[j]) + 4; s.ldc2 = pad4(N2[j]) + 12; }
    if (mode == 2) { s.ldb2 = N2[j]; s.ldc2 = N2[j]; }
    run_case(s); });
  // g1a: dW_in += W_ih0^T Z with ldc = nin = 65 / 475, split-K (small tiles: never on the x3 kernel)
  if (!elig) lattice(10, 2, 12, [&](int i, int j, int k, int r) {
    Spec s; s.form = "g1a"; s.akc = s.bkc = false; s.M = MN[i]; s.N = j ? 475 : 65; s.K = KSK[k][0]; s.sk = KSK[k][1];
    s.fb = -1; s.beta = 1; s.slab = pick(r, 2, 2);
    s.lda = pad4(s.M); s.ldb = (s.N + 3) / 4 * 4; s.ldc = s.N; run_case(s); });
}

int main(int argc, char** argv) {
  tally.args(argc, argv);
  if (!tally.plan_mode) arena.init();
  all_cases(false);
  all_cases(true);
  if (!tally.plan_mode) for (const std::string& f : form_order) { const FormStat& fs = stats[f];
    printf("worst fraction of the bound  %-24s exact kernel %.3f   x3 kernel %.3f   (%d cases, %d failed)\n", f.c_str(), fs.frac, fs.frac_x3, fs.cases, fs.fails); }
  return tally.finish("GEMM");
}
