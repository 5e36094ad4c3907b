// Step-wise check of every LSTM recurrence kernel (kbj_lstm_seq.h, kbj_lstm_bwd16.h) against a double-precision reference.
//   make -C tools lstm_check && tools/lstm_check            (GPU; ends with LSTM CHECK PASSED or a non-zero exit status)
//   tools/lstm_check --plan                                  (no device: the same case table; proves what the checker accepts and rejects)
// Every launch goes through the launch helpers of the two headers (seq_fwd_launch, seq_bwd_launch, seq_bwd16_launch, lstm_step_launch),
// the ones kbj_nn.hip calls: hidden-size dispatch, grid and workgroup-to-tile mapping are under test with the kernels. No timing.
//
// METHOD: TEACHER-FORCED STEPS PLUS EXACT LINKS. Every step t is compared with a double reference computed from what the kernel ITSELF
// stored as that step's inputs (Hm[t], Cm[t], resp. dG[t+1]); the links between steps are demanded bit for bit. A chain whose every step
// and every link is right is right as a whole, rounding does not compound over t, so the bounds stay near 1e-6 while an indexing error
// (wrong row, unit, gate, step, keep flag) shows as O(1). u = 2^-24, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical
// Algorithms, section 3.1: n roundings in any order), the double reference's own error (1e-9 of the same sums) is added.
//
// ACTIVATIONS (C_sig, C_tanh). The kernels' comment relies on v_exp_f32 and v_rcp_f32 being "1 ULP" instructions, which is what AMD documents
// ("AMD Instinct MI300 Instruction Set Architecture Reference Guide", V_EXP_F32 and V_RCP_F32: 1 ULP accuracy; the LLVM AMDGPU usage guide
// says the same of llvm.amdgcn.rcp). One ulp is at most 2 u relative.
//   seq_sigmoid(x) = rcp(1 + exp2(fl(-x log2e))): the scaled argument y carries two roundings (the constant's and the product's), |dy| <= 2 u |y|,
//   which exp2 turns into a relative error ln2 |dy| = 2 u |x| of e = exp(-x); with the instruction's own 2 u: e (1 + d), |d| <= 2 u (|x| + 1).
//   s = 1 / (1 + e) has ds/de = -s^2, so the absolute error from e is s (1 - s) |d| <= 2 u (max |x| s (1 - s) + max s (1 - s)) =
//   2 u (0.2239 + 0.25) < 0.95 u. The addition 1 + e rounds once (relative u, hence <= u s <= u absolute), rcp adds 2 u s <= 2 u.
//   |seq_sigmoid - sigmoid| <= 3.95 u:   C_sig = 4.
//   seq_tanh(x) = 1 - 2 rcp(1 + exp2(fl(2 xc log2e))), xc = x clamped to +-15 (tanh(15) = 1 - 1.9e-13: the clamp costs < 1e-12, 2 xc is exact).
//   r = rcp(...) as above with z = 2 x: <= 0.95 u + 3 u r <= 3.95 u; doubling is exact, the final subtraction rounds once (<= u):
//   |seq_tanh - tanh| <= 2 x 3.95 u + u = 8.9 u:   C_tanh = 9.
// These are worst cases over all x; they are NOT tuned to a run. The tool prints the worst seq_tanh error it can observe in isolation
// (TanhC[t] against tanh of the stored Cm[t+1] where keep = 1, the very fp32 number the kernel fed to seq_tanh) and holds it to C_tanh u.
//
// FORWARD, for every t, row r < B, unit:
//   gate activations G[t] against sigmoid / tanh of the double pre-activation p = G_in[t] (or bias + x_t W_ih^T over the kx valid columns)
//     + Hm[t] W_hh^T, Hm[t] from the implementation under test:  |act - ref| <= L gamma_n sum|terms| + C u,  L = 1/4 (sigmoid), 1 (tanh),
//     n = H + 2 (plain), H + KX + 1 (fused forms);
//   Cm[t+1] against keep_t (f Cm[t] + i g) with the implementation's own i, f, g:  <= 3 u (|f Cm| + |i g|)  (two products and a sum, or a
//     product and a fused multiply-add: at most u per product and u on the sum, rounded up for second order; the keep product is exact);
//   TanhC[t] against tanh of that double c:  <= C_tanh u + 3 u (|f Cm| + |i g|)  (|tanh'| <= 1);
//   Hout[t] == fl(o TanhC[t]) and Hm[t+1] == fl(Hout[t] keep_t): single fp32 products of stored values, BIT FOR BIT;
//   slot 0 of Hm and Cm unchanged, bit for bit.
//   One free-running comparison of Hout with the all-double recurrence is printed (worst absolute error), not asserted.
// STEP KERNEL (gates are not stored): with e_k = L gamma_n sum|terms| + C u per gate, C against c = f Cprev + i g within
//   e_c = |Cprev| e_f + |g| e_i + |i| e_g + e_i e_g + 3 u (|f Cprev| + |i g|), Hout against o tanh(c) within e_o (|tanh c| + C_tanh u + e_c)
//   + |o| (C_tanh u + e_c) + u |h|; Hin unchanged bit for bit.
// BACKWARD, both tilings, t downwards, with the implementation's own dG[t+1]:
//   dhm = dG[t+1] W_hh (K = 4H fused multiply-adds and at most 3 additions of partial sums): error E = gamma_{4H+3} sum|terms|.
//   dh = dHabove + keep dhm:        e_dh = keep E + u |dh|
//   w = 1 - tc^2 (two roundings, absolute error <= u since tc^2 + w = 1), q = dh o w:   e_q = e_dh |o w| + u |dh o| + 2 u |q|
//   dc = keep dcm + q:              e_dc = keep e_dcm + e_q + u |dc|          (the cell gradient lives in registers only: the reference carries
//   dcm' = dc f:                    e_dcm' = e_dc f + u |dcm'|                 dc, dcm in double and this bound beside it; f keep <= 1, so the
//                                                                              chain's own error never amplifies)
//   d0 = dc g i (1 - i):            e_dc |g i (1 - i)| + 4 u |d0|             (three products and the rounding of 1 - i)
//   d1 = dc Cm[t] f (1 - f):        e_dc |Cm f (1 - f)| + 4 u |d1|
//   d2 = dc i (1 - g^2):            e_dc |i (1 - g^2)| + u |dc i| + 3 u |d2|
//   d3 = dh tc o (1 - o):           e_dh |tc o (1 - o)| + 4 u |d3|
//   every bound x 1.01 for the second-order terms, + 1e-35 (products below the normal range may be flushed).
//   db (atomics): against db0 + the double column sums of the implementation's own dG within gamma_{T B + 1} (|db0| + sum |dG|).
//   db_part (deterministic mode): per (row, gate, unit) the fp32 chain over t descending from 0, then the row group's rows ascending from 0,
//   rows beyond B contributing zero - reproduced on the host from the stored dG and demanded BIT FOR BIT. The array has exactly
//   ceil(B / rows) rows between its guards: a grid with a row group too many writes into a guard.
//
// HARNESS (tools/kbj_check.h: the arena, the guarded window, the tally). Every array is a window, inputs between NaN and outputs between
// the bit pattern; pure outputs start as NaN (an element nobody wrote fails its check). Where kx < KX the columns kx..ldx of X are NaN and the
// weight columns there hold +-1000: the result must see neither. Counters and the error word are zeroed before each launch. Before a
// recurrence launch the grid must be resident (seq_blocks_per_cu of kbj_lstm_bwd16.h, the library's own occupancy table, x CUs) and at most
// 64 workgroups, else the case FAILs without a launch; the step kernel never waits for another workgroup and runs the library's own grid
// (up to 256). A set error word or any HIP error ends the run at once.
//
// --plan (no device). Per case: (1) at least 90 % of the double reference's gate pre-activations have |x| <= 3 (a saturated gate hides a wrong
// recurrent term); (2) the checker passes a host fp32 model of the kernel (plain loops from the Args comments, expf and a division);
// (3) the checker rejects every mutant of that model, by more than 100 x the bound in at least one element, in every case that exercises the
// mutated feature (`exercised` below: a rule on the case's parameters, mirrored by tests/test_gpu_lstm_check.py); other cases say n/a.
#include <atomic>
#include <thread>
#include "kbj_check.h"
#include "kbj_lstm_seq.h"
#include "kbj_lstm_bwd16.h"

using namespace kbj;

static void fill(std::vector<float>& v, size_t n, uint32_t tag, float scale) { v.resize(n); for (size_t i = 0; i < n; ++i) v[i] = scale * val_real(hash3(tag, (uint32_t)(i >> 16), (uint32_t)(i & 0xFFFF))); }

constexpr double C_SIG = 4.0, C_TANH = 9.0, REF_ERR = 1e-9, SECOND_ORDER = 1.01, FLUSH = 1e-35;
static double sigm(double x) { return 1.0 / (1.0 + std::exp(-x)); }

template <class F> static void par_for(int n, F f) {
  static const int nt = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (n < 2 || nt < 2) { for (int i = 0; i < n; ++i) f(i); return; }
  std::atomic<int> next{0};
  std::vector<std::thread> th;
  for (int k = 0; k < std::min(nt, n); ++k) th.emplace_back([&] { for (int i; (i = next.fetch_add(1)) < n;) f(i); });
  for (auto& t : th) t.join();
}
// s += sum x[k] w[k], a += sum |x[k] w[k]| in double (four chains: the order of a double sum is free at these bounds)
template <class TX> static void dot(const TX* x, const float* w, int n, double& s, double& a) {
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0, a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  int k = 0;
  for (; k + 4 <= n; k += 4) {
    const double p0 = (double)x[k] * w[k], p1 = (double)x[k + 1] * w[k + 1], p2 = (double)x[k + 2] * w[k + 2], p3 = (double)x[k + 3] * w[k + 3];
    s0 += p0; s1 += p1; s2 += p2; s3 += p3; a0 += std::fabs(p0); a1 += std::fabs(p1); a2 += std::fabs(p2); a3 += std::fabs(p3);
  }
  for (; k < n; ++k) { const double p = (double)x[k] * w[k]; s0 += p; a0 += std::fabs(p); }
  s += (s0 + s1) + (s2 + s3); a += (a0 + a1) + (a2 + a3);
}
static float dotf(const float* x, const float* w, int n) {
  float s0 = 0, s1 = 0, s2 = 0, s3 = 0; int k = 0;
  for (; k + 4 <= n; k += 4) { s0 += x[k] * w[k]; s1 += x[k + 1] * w[k + 1]; s2 += x[k + 2] * w[k + 2]; s3 += x[k + 3] * w[k + 3]; }
  for (; k < n; ++k) s0 += x[k] * w[k];
  return (s0 + s1) + (s2 + s3);
}

// ---- cases ---------------------------------------------------------------------------------------------------------------------------
enum Form { PLAIN = 0, FUSED = 1, OBS = 2 };
enum Keep { K_ONES = 0, K_ZEROS, K_T0, K_TLAST, K_HASH, NKEEP };
static const char* KEEPN[NKEEP] = {"ones", "zeros", "t0", "tlast", "hashed"};
enum Mut { M_NONE = 0, M_KEEP_IGN, M_KEEP_NBR, M_CM_UNMASKED, M_KX, M_DC_KEEP_NEXT, M_DH_UNMASKED, M_CPREV, M_DBPART_TREE, NMUT };
static const char* MUTN[NMUT] = {"", "keep_ignored", "keep_neighbour", "cm_unmasked", "kx_beyond", "dc_keep_next", "dh_unmasked", "cprev_next", "dbpart_pairwise"};
enum Family { FAM_FWD, FAM_BWD, FAM_STEP };
static const int FAM_MUTS[3][7] = {{M_KEEP_IGN, M_KEEP_NBR, M_CM_UNMASKED, M_KX, 0, 0, 0},
                                   {M_KEEP_IGN, M_KEEP_NBR, M_DC_KEEP_NEXT, M_DH_UNMASKED, M_CPREV, M_DBPART_TREE, 0},
                                   {M_KX, 0, 0, 0, 0, 0, 0}};
// does a case exercise what the mutant breaks? (a rule on the parameters; the hashed keep pattern pins keep[0][row 0] = 0, keep[1][row 0] = 1)
static bool exercised(int fam, int mut, int T, int keep, int B, bool kx_short, bool part) {
  const bool differs_in_t = T >= 2 && (keep == K_T0 || keep == K_TLAST || keep == K_HASH);      // some row's keep differs between neighbouring steps
  const bool zero_before_last = T >= 2 && (keep == K_ZEROS || keep == K_T0 || keep == K_HASH);  // a zero at some t < T - 1 (the last step has nothing recurrent to mask in BPTT)
  switch (mut) {
    case M_KEEP_IGN: return fam == FAM_FWD ? keep != K_ONES : zero_before_last;
    case M_KEEP_NBR: return differs_in_t;
    case M_CM_UNMASKED: return keep != K_ONES;
    case M_KX: return kx_short;
    case M_DC_KEEP_NEXT: return differs_in_t;
    case M_DH_UNMASKED: return zero_before_last;
    case M_CPREV: return true;
    case M_DBPART_TREE: return part && B >= 3;      // a tree over fewer than three non-zero rows is the chain
  }
  return false;
}
static void make_keep(std::vector<float>& keep, int T, int B, int pat, uint32_t tag) {
  keep.assign((size_t)T * B, 1.0f);
  for (int t = 0; t < T; ++t) for (int r = 0; r < B; ++r) {
    float& k = keep[(size_t)t * B + r];
    if (pat == K_ZEROS) k = 0.0f;
    else if (pat == K_T0) k = t == 0 ? 0.0f : 1.0f;
    else if (pat == K_TLAST) k = t == T - 1 ? 0.0f : 1.0f;
    else if (pat == K_HASH) k = hash3(tag, t, r) % 10u < 3u ? 0.0f : 1.0f;
  }
  if (pat == K_HASH) { keep[0] = 0.0f; if (T >= 2) keep[B] = 1.0f; }
}
static int neighbour(int t, int T) { return t + 1 < T ? t + 1 : (t > 0 ? t - 1 : t); }

// one forward problem (also the step kernel: T = 1, keep = 1, Hm[0] = Hin, Cm[0] = C before, Cm[1] = C after)
struct Fwd {
  int H = 0, B = 0, T = 0, form = PLAIN, KX = 0, ld = 0, kx = 0;   // ld = ldx = ldw; kx = valid input columns (= KX unless the case shortens it)
  std::vector<float> Gin, X, Wih, bias, Whh, keep, H0, C0;         // inputs
  std::vector<float> G, Hm, Cm, Hout, TanhC;                        // outputs of the implementation under test
  size_t bh() const { return (size_t)B * H; }
};
static void make_fwd(Fwd& p, int H, int B, int T, int form, int kx, int keep_pat, uint32_t id) {
  p.H = H; p.B = B; p.T = T; p.form = form;
  p.KX = form == OBS ? KBJ_LD_ACTOR : H; p.ld = p.KX; p.kx = kx ? kx : p.KX;
  const uint32_t tag = id * 16u;
  fill(p.Whh, (size_t)4 * H * H, tag + 1, 1.0f / std::sqrt((float)H));
  fill(p.H0, p.bh(), tag + 2, 1.0f); fill(p.C0, p.bh(), tag + 3, 1.0f);
  make_keep(p.keep, T, B, keep_pat, tag + 4);
  if (form == PLAIN) fill(p.Gin, (size_t)T * B * 4 * H, tag + 5, 1.0f);
  else {
    fill(p.X, (size_t)T * B * p.ld, tag + 6, 1.0f);
    fill(p.Wih, (size_t)4 * H * p.ld, tag + 7, 1.0f / std::sqrt((float)p.KX));
    fill(p.bias, (size_t)4 * H, tag + 8, 0.5f);
    for (size_t row = 0; row < (size_t)T * B; ++row) for (int c = p.kx; c < p.ld; ++c) p.X[row * p.ld + c] = QNAN;
    for (int row = 0; row < 4 * H; ++row) for (int c = p.kx; c < p.ld; ++c) p.Wih[(size_t)row * p.ld + c] *= 1000.0f * std::sqrt((float)p.KX);
  }
}
// double pre-activations of row r at step t (all 4H) from the stored inputs and the h row, with the sum of |terms|
template <class TH> static void preact(const Fwd& p, int t, int r, const TH* h, double* pre, double* sab) {
  const int H = p.H;
  for (int j = 0; j < 4 * H; ++j) {
    double s, a;
    if (p.form == PLAIN) { s = p.Gin[((size_t)t * p.B + r) * 4 * H + j]; a = std::fabs(s); }
    else { s = p.bias[j]; a = std::fabs(s); dot(&p.X[((size_t)t * p.B + r) * p.ld], &p.Wih[(size_t)j * p.ld], p.kx, s, a); }
    dot(h, &p.Whh[(size_t)j * H], H, s, a);
    pre[j] = s; sab[j] = a;
  }
}
// the all-double recurrence (free running): reference of the free-running figure, source of the backward cases' stored activations
struct FwdRef { std::vector<double> G, Hm, Cm, Hout, TanhC; double alive = 0; };
static void ref_fwd(const Fwd& p, FwdRef& o) {
  const int H = p.H, B = p.B, T = p.T;
  o.G.assign((size_t)T * B * 4 * H, 0); o.Hm.assign((size_t)(T + 1) * p.bh(), 0); o.Cm = o.Hm; o.Hout.assign((size_t)T * p.bh(), 0); o.TanhC = o.Hout;
  for (size_t i = 0; i < p.bh(); ++i) { o.Hm[i] = p.H0[i]; o.Cm[i] = p.C0[i]; }
  std::vector<long> live(B, 0);
  par_for(B, [&](int r) {
    std::vector<double> pre(4 * H), sab(4 * H);
    for (int t = 0; t < T; ++t) {
      const size_t o0 = (size_t)t * p.bh() + (size_t)r * H, o1 = o0 + p.bh();
      preact(p, t, r, &o.Hm[o0], pre.data(), sab.data());
      const double kp = p.keep[(size_t)t * B + r];
      for (int j = 0; j < 4 * H; ++j) live[r] += std::fabs(pre[j]) <= 3.0;
      for (int u = 0; u < H; ++u) {
        const double ig = sigm(pre[u]), fg = sigm(pre[H + u]), gg = std::tanh(pre[2 * H + u]), og = sigm(pre[3 * H + u]);
        double* g = &o.G[((size_t)t * B + r) * 4 * H + u];
        g[0] = ig; g[H] = fg; g[2 * H] = gg; g[3 * H] = og;
        const double c = fg * o.Cm[o0 + u] + ig * gg, tc = std::tanh(c), h = og * tc;
        o.TanhC[o0 + u] = tc; o.Hout[o0 + u] = h; o.Cm[o1 + u] = c * kp; o.Hm[o1 + u] = h * kp;
      }
    }
  });
  long n = 0; for (long v : live) n += v;
  o.alive = (double)n / ((double)T * B * 4 * H);
}
static float sigf(float x) { return 1.0f / (1.0f + expf(-x)); }
static float tanhf_(float x) { return 1.0f - 2.0f / (1.0f + expf(2.0f * x)); }
// host fp32 model of lstm_seq_fwd_kernel / lstm_step_kernel from the Args comments, and its mutants
static void model_fwd(Fwd& p, int mut) {
  const int H = p.H, B = p.B, T = p.T;
  p.G.assign((size_t)T * B * 4 * H, QNAN); p.Hm.assign((size_t)(T + 1) * p.bh(), QNAN); p.Cm = p.Hm; p.Hout.assign((size_t)T * p.bh(), QNAN); p.TanhC = p.Hout;
  std::copy(p.H0.begin(), p.H0.end(), p.Hm.begin()); std::copy(p.C0.begin(), p.C0.end(), p.Cm.begin());
  const int kcols = mut == M_KX ? p.KX : p.kx;
  par_for(B, [&](int r) {
    std::vector<float> pre(4 * H);
    for (int t = 0; t < T; ++t) {
      const size_t o0 = (size_t)t * p.bh() + (size_t)r * H, o1 = o0 + p.bh();
      for (int j = 0; j < 4 * H; ++j) {
        float s = p.form == PLAIN ? p.Gin[((size_t)t * B + r) * 4 * H + j] : p.bias[j] + dotf(&p.X[((size_t)t * B + r) * p.ld], &p.Wih[(size_t)j * p.ld], kcols);
        pre[j] = s + dotf(&p.Hm[o0], &p.Whh[(size_t)j * H], H);
      }
      float kp = p.keep[(size_t)(mut == M_KEEP_NBR ? neighbour(t, T) : t) * B + r];
      if (mut == M_KEEP_IGN) kp = 1.0f;
      for (int u = 0; u < H; ++u) {
        const float ig = sigf(pre[u]), fg = sigf(pre[H + u]), gg = tanhf_(pre[2 * H + u]), og = sigf(pre[3 * H + u]);
        float* g = &p.G[((size_t)t * B + r) * 4 * H + u];
        g[0] = ig; g[H] = fg; g[2 * H] = gg; g[3 * H] = og;
        const float c = fg * p.Cm[o0 + u] + ig * gg, tc = tanhf_(c), h = og * tc;
        p.TanhC[o0 + u] = tc; p.Hout[o0 + u] = h; p.Hm[o1 + u] = h * kp; p.Cm[o1 + u] = mut == M_CM_UNMASKED ? c : c * kp;
      }
    }
  });
}

// ---- the checker's bookkeeping -----------------------------------------------------------------------------------------------------------
enum Cat { C_ACT = 0, C_CELL, C_TANHC, C_TANH_PURE, C_LINK, C_DG, C_DB, C_DBPART, C_STEP_C, C_STEP_H, NCAT };
static const char* CATN[NCAT] = {"act", "c", "tanhc", "seq_tanh", "links", "dG", "db", "db_part", "C", "Hout"};
static std::atomic<bool> early_exit{false}, rejected{false};   // plan mode, mutants: the first element beyond 100 x its bound settles the case
struct Chk {
  double worst[NCAT]; bool seen[NCAT]; double tanh_pure_u = 0; char why[160];
  Chk() { for (int i = 0; i < NCAT; ++i) { worst[i] = 0; seen[i] = false; } why[0] = 0; }
  // err against bound (a NaN fails); exact checks pass err = 0 or infinity with bound = 0
  void upd(int cat, double err, double bound, int t, int r, int gate, int unit) {
    double ratio = err == 0.0 ? 0.0 : (err <= bound ? err / bound : (bound > 0 && err == err ? err / bound : INFINITY));
    seen[cat] = true;
    if (ratio > 100.0 && early_exit.load(std::memory_order_relaxed)) rejected.store(true, std::memory_order_relaxed);
    if (ratio > worst[cat]) {
      if (ratio > 1.0 && max_ratio() <= 1.0) snprintf(why, sizeof why, "%s t=%d row=%d gate=%d unit=%d err %.3g bound %.3g", CATN[cat], t, r, gate, unit, err, bound);
      worst[cat] = ratio;
    }
  }
  void exact(int cat, float got, float want, int t, int r, int gate, int unit) { upd(cat, same_bits(got, want) ? 0.0 : INFINITY, 0.0, t, r, gate, unit); }
  double max_ratio() const { double m = 0; for (int i = 0; i < NCAT; ++i) m = std::max(m, worst[i]); return m; }
  void merge(const Chk& o) {
    if (o.max_ratio() > 1.0 && max_ratio() <= 1.0) memcpy(why, o.why, sizeof why);
    for (int i = 0; i < NCAT; ++i) { worst[i] = std::max(worst[i], o.worst[i]); seen[i] = seen[i] || o.seen[i]; }
    tanh_pure_u = std::max(tanh_pure_u, o.tanh_pure_u);
  }
};
static Chk merged(const std::vector<Chk>& v) { Chk c; for (const Chk& x : v) c.merge(x); return c; }

static Chk check_fwd(const Fwd& p) {
  const int H = p.H, B = p.B, T = p.T;
  const double g_n = gamma_n(p.form == PLAIN ? H + 2 : H + p.KX + 1) + REF_ERR;
  std::vector<Chk> rows(B);
  par_for(B, [&](int r) {
    Chk& k = rows[r];
    if (rejected.load(std::memory_order_relaxed)) return;
    std::vector<double> pre(4 * H), sab(4 * H);
    for (int u = 0; u < H; ++u) { k.exact(C_LINK, p.Hm[(size_t)r * H + u], p.H0[(size_t)r * H + u], -1, r, -1, u); k.exact(C_LINK, p.Cm[(size_t)r * H + u], p.C0[(size_t)r * H + u], -1, r, -2, u); }
    for (int t = 0; t < T; ++t) {
      const size_t o0 = (size_t)t * p.bh() + (size_t)r * H, o1 = o0 + p.bh();
      preact(p, t, r, &p.Hm[o0], pre.data(), sab.data());
      const float kp = p.keep[(size_t)t * B + r];
      const float* g = &p.G[((size_t)t * B + r) * 4 * H];
      for (int u = 0; u < H; ++u) {
        for (int gate = 0; gate < 4; ++gate) {
          const int j = gate * H + u;
          const double ref = gate == 2 ? std::tanh(pre[j]) : sigm(pre[j]);
          k.upd(C_ACT, std::fabs(g[j] - ref), (gate == 2 ? 1.0 : 0.25) * g_n * sab[j] + (gate == 2 ? C_TANH : C_SIG) * U, t, r, gate, u);
        }
        const double ig = g[u], fg = g[H + u], gg = g[2 * H + u], og = g[3 * H + u], cm = p.Cm[o0 + u];
        const double c = fg * cm + ig * gg, mag = std::fabs(fg * cm) + std::fabs(ig * gg);
        k.upd(C_CELL, std::fabs(p.Cm[o1 + u] - kp * c), 3 * U * mag, t, r, -1, u);
        k.upd(C_TANHC, std::fabs(p.TanhC[o0 + u] - std::tanh(c)), C_TANH * U + 3 * U * mag, t, r, -1, u);
        if (kp == 1.0f) {   // Cm[t+1] IS the fp32 c that went into seq_tanh
          const double e = std::fabs(p.TanhC[o0 + u] - std::tanh((double)p.Cm[o1 + u]));
          k.upd(C_TANH_PURE, e, C_TANH * U, t, r, -1, u);
          if (e == e) k.tanh_pure_u = std::max(k.tanh_pure_u, e / U);
        }
        k.exact(C_LINK, p.Hout[o0 + u], (float)og * p.TanhC[o0 + u], t, r, 3, u);
        k.exact(C_LINK, p.Hm[o1 + u], p.Hout[o0 + u] * kp, t, r, 4, u);
      }
    }
  });
  return merged(rows);
}
static double free_running_error(const Fwd& p, const FwdRef& ref) {
  double w = 0;
  for (size_t i = 0; i < p.Hout.size(); ++i) { const double e = std::fabs(p.Hout[i] - ref.Hout[i]); w = e == e ? std::max(w, e) : INFINITY; }
  return w;
}
static Chk check_step(const Fwd& p) {   // outputs used: Hout [M][H], Cm slot 1 = C after; Hm slot 0 = Hin as the implementation left it
  const int H = p.H, M = p.B;
  const double g_n = gamma_n(H + p.KX + 1) + REF_ERR;
  std::vector<Chk> rows(M);
  par_for(M, [&](int r) {
    Chk& k = rows[r];
    if (rejected.load(std::memory_order_relaxed)) return;
    std::vector<double> pre(4 * H), sab(4 * H);
    preact(p, 0, r, &p.H0[(size_t)r * H], pre.data(), sab.data());
    for (int u = 0; u < H; ++u) {
      k.exact(C_LINK, p.Hm[(size_t)r * H + u], p.H0[(size_t)r * H + u], 0, r, -1, u);
      const double ig = sigm(pre[u]), fg = sigm(pre[H + u]), gg = std::tanh(pre[2 * H + u]), og = sigm(pre[3 * H + u]);
      const double ei = 0.25 * g_n * sab[u] + C_SIG * U, ef = 0.25 * g_n * sab[H + u] + C_SIG * U, eg = g_n * sab[2 * H + u] + C_TANH * U, eo = 0.25 * g_n * sab[3 * H + u] + C_SIG * U;
      const double cp = p.C0[(size_t)r * H + u], c = fg * cp + ig * gg, mag = std::fabs(fg * cp) + std::fabs(ig * gg);
      const double ec = std::fabs(cp) * ef + std::fabs(gg) * ei + ig * eg + ei * eg + 3 * U * mag;
      k.upd(C_STEP_C, std::fabs(p.Cm[p.bh() + (size_t)r * H + u] - c), SECOND_ORDER * ec, 0, r, -1, u);
      const double tc = std::tanh(c), h = og * tc;
      k.upd(C_STEP_H, std::fabs(p.Hout[(size_t)r * H + u] - h), SECOND_ORDER * (eo * (std::fabs(tc) + C_TANH * U + ec) + og * (C_TANH * U + ec) + U * std::fabs(h)), 0, r, -1, u);
    }
  });
  return merged(rows);
}
static void model_step(Fwd& p, int mut) {   // the cell of the inputs; Hin (Hm slot 0) untouched, Cm slot 1 = the updated C
  model_fwd(p, mut);
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
struct Bwd {
  int H = 0, B = 0, T = 0, rows = SEQ_ROWS; bool part = false;     // rows per row group: 32 or 16
  std::vector<float> Gact, TanhC, Cm, dHa, keep, Whh, WhhT, db0;    // inputs (WhhT [H][4H]: host-side transpose for the reference)
  std::vector<float> dG, db, db_part;                               // outputs
  int nrg() const { return (B + rows - 1) / rows; }
  size_t bh() const { return (size_t)B * H; }
};
static double make_bwd(Bwd& q, int H, int B, int T, int rows, bool part, int keep_pat, uint32_t id) {   // returns the forward reference's live-gate fraction
  Fwd p; make_fwd(p, H, B, T, PLAIN, 0, keep_pat, id);
  FwdRef f; ref_fwd(p, f);
  q.H = H; q.B = B; q.T = T; q.rows = rows; q.part = part;
  q.Gact.assign(f.G.begin(), f.G.end()); q.TanhC.assign(f.TanhC.begin(), f.TanhC.end()); q.Cm.assign(f.Cm.begin(), f.Cm.end());
  q.keep = p.keep; q.Whh = p.Whh;
  q.WhhT.resize(q.Whh.size());
  for (int k = 0; k < 4 * H; ++k) for (int u = 0; u < H; ++u) q.WhhT[(size_t)u * 4 * H + k] = q.Whh[(size_t)k * H + u];
  fill(q.dHa, (size_t)T * q.bh(), id * 16u + 9, 1.0f);
  fill(q.db0, (size_t)4 * H, id * 16u + 10, 1.0f);
  return f.alive;
}
// per-row-group bias partials from a stored dG, in the documented order or with the rows added pairwise
static void db_part_of(const Bwd& q, const std::vector<float>& dG, bool pairwise, std::vector<float>& out) {
  const int H = q.H, B = q.B, T = q.T, R = q.rows;
  out.assign((size_t)q.nrg() * 4 * H, 0.0f);
  par_for(q.nrg(), [&](int rg) {
    std::vector<float> col(R);
    for (int j = 0; j < 4 * H; ++j) {
      for (int i = 0; i < R; ++i) {
        const int r = rg * R + i; float s = 0.0f;
        if (r < B) for (int t = T - 1; t >= 0; --t) s += dG[((size_t)t * B + r) * 4 * H + j];
        col[i] = s;
      }
      out[(size_t)rg * 4 * H + j] = pairwise ? tree(col.data(), R, 1) : chain(col.data(), R, 1);
    }
  });
}
static void model_bwd(Bwd& q, int mut) {
  const int H = q.H, B = q.B, T = q.T;
  q.dG.assign((size_t)T * B * 4 * H, QNAN);
  par_for(B, [&](int r) {
    std::vector<float> dcm(H, 0.0f);
    for (int t = T - 1; t >= 0; --t) {
      float kp = q.keep[(size_t)(mut == M_KEEP_NBR ? neighbour(t, T) : t) * B + r];
      if (mut == M_KEEP_IGN) kp = 1.0f;
      const float kp_dh = mut == M_DH_UNMASKED ? 1.0f : kp;
      const float kp_dc = mut == M_DC_KEEP_NEXT ? (t + 1 < T ? q.keep[(size_t)(t + 1) * B + r] : kp) : kp;
      for (int u = 0; u < H; ++u) {
        const float dhm = t + 1 < T ? dotf(&q.dG[((size_t)(t + 1) * B + r) * 4 * H], &q.WhhT[(size_t)u * 4 * H], 4 * H) : 0.0f;
        const size_t o1 = (size_t)t * q.bh() + (size_t)r * H + u;
        const float* g = &q.Gact[((size_t)t * B + r) * 4 * H + u];
        const float ig = g[0], fg = g[H], gg = g[2 * H], og = g[3 * H], tc = q.TanhC[o1], cprev = q.Cm[mut == M_CPREV ? o1 + q.bh() : o1];
        const float dh = q.dHa[o1] + kp_dh * dhm;
        const float dc = kp_dc * dcm[u] + dh * og * (1 - tc * tc);
        float* d = &q.dG[((size_t)t * B + r) * 4 * H + u];
        d[0] = dc * gg * ig * (1 - ig); d[H] = dc * cprev * fg * (1 - fg); d[2 * H] = dc * ig * (1 - gg * gg); d[3 * H] = dh * tc * og * (1 - og);
        dcm[u] = dc * fg;
      }
    }
  });
  if (q.part) db_part_of(q, q.dG, mut == M_DBPART_TREE, q.db_part);
  else {
    q.db = q.db0;
    for (int j = 0; j < 4 * H; ++j) { float s = 0; for (size_t row = 0; row < (size_t)T * B; ++row) s += q.dG[row * 4 * H + j]; q.db[j] += s; }
  }
}
static Chk check_bwd(const Bwd& q) {
  const int H = q.H, B = q.B, T = q.T;
  const double g_k = gamma_n(4 * H + 3) + REF_ERR;
  std::vector<Chk> rows(B);
  par_for(B, [&](int r) {
    Chk& k = rows[r];
    std::vector<double> dcm(H, 0.0), edcm(H, 0.0);
    for (int t = T - 1; t >= 0 && !rejected.load(std::memory_order_relaxed); --t) {
      const double kp = q.keep[(size_t)t * B + r];
      for (int u = 0; u < H; ++u) {
        double dhm = 0, S = 0;
        if (t + 1 < T) dot(&q.dG[((size_t)(t + 1) * B + r) * 4 * H], &q.WhhT[(size_t)u * 4 * H], 4 * H, dhm, S);
        const size_t o1 = (size_t)t * q.bh() + (size_t)r * H + u;
        const float* g = &q.Gact[((size_t)t * B + r) * 4 * H + u];
        const double ig = g[0], fg = g[H], gg = g[2 * H], og = g[3 * H], tc = q.TanhC[o1], cprev = q.Cm[o1];
        const double dh = q.dHa[o1] + kp * dhm, edh = kp * g_k * S + U * std::fabs(dh);
        const double w = 1 - tc * tc, qq = dh * og * w, eq = edh * std::fabs(og * w) + U * std::fabs(dh * og) + 2 * U * std::fabs(qq);
        const double dc = kp * dcm[u] + qq, edc = kp * edcm[u] + eq + U * std::fabs(dc);
        const double d[4] = {dc * gg * ig * (1 - ig), dc * cprev * fg * (1 - fg), dc * ig * (1 - gg * gg), dh * tc * og * (1 - og)};
        const double e[4] = {edc * std::fabs(gg * ig * (1 - ig)) + 4 * U * std::fabs(d[0]), edc * std::fabs(cprev * fg * (1 - fg)) + 4 * U * std::fabs(d[1]),
                             edc * std::fabs(ig * (1 - gg * gg)) + U * std::fabs(dc * ig) + 3 * U * std::fabs(d[2]), edh * std::fabs(tc * og * (1 - og)) + 4 * U * std::fabs(d[3])};
        const float* got = &q.dG[((size_t)t * B + r) * 4 * H + u];
        for (int gate = 0; gate < 4; ++gate) k.upd(C_DG, std::fabs(got[gate * H] - d[gate]), SECOND_ORDER * e[gate] + FLUSH, t, r, gate, u);
        dcm[u] = dc * fg; edcm[u] = edc * fg + U * std::fabs(dcm[u]);
      }
    }
  });
  Chk k = merged(rows);
  if (q.part) {
    std::vector<float> want; db_part_of(q, q.dG, false, want);
    if (want.size() != q.db_part.size()) k.upd(C_DBPART, INFINITY, 0, -1, -1, -1, -1);
    else for (size_t i = 0; i < want.size(); ++i) k.exact(C_DBPART, q.db_part[i], want[i], -1, (int)(i / (4 * H)), (int)(i % (4 * H)) / H, (int)(i % H));
  } else {
    const double g_b = gamma_n(T * B + 1) + REF_ERR;
    for (int j = 0; j < 4 * H; ++j) {
      double s = q.db0[j], a = std::fabs(s);
      for (size_t row = 0; row < (size_t)T * B; ++row) { const double v = q.dG[row * 4 * H + j]; s += v; a += std::fabs(v); }
      k.upd(C_DB, std::fabs(q.db[j] - s), g_b * a + FLUSH, -1, -1, j / H, j % H);
    }
  }
  return k;
}

// ---- device side ---------------------------------------------------------------------------------------------------------------------------
static Arena arena((size_t)96 << 20);
static int n_cus = 0; static unsigned timeout_ticks = 0; static unsigned* sync_words = nullptr;   // [256 counters][error word]
static bool resident(SeqKernelKind kind, int H, int grid, char* why, size_t nwhy) {
  if (grid > 64) { snprintf(why, nwhy, "grid %d above the tool's 64 workgroups: not launched", grid); return false; }
  int per_cu = 0;
  if (seq_blocks_per_cu(kind, H, &per_cu) != hipSuccess) per_cu = 0;   // not built for this hidden size: no slots
  const long slots = (long)per_cu * n_cus;
  if (grid > slots) { snprintf(why, nwhy, "grid %d not resident (%ld slots): not launched", grid, slots); return false; }
  return true;
}
static void prepare_launch() { CK(hipMemset(sync_words, 0, 257 * sizeof(unsigned))); }
// after a launch: any HIP error or a set error word ends the run (nothing further is launched)
static void finish_launch(const char* kernel, const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned err = 0;
  if (e == hipSuccess) e = hipMemcpy(&err, sync_words + 256, 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess || err) {
    printf("case %-10s %-40s : FAIL %s\n", kernel, what, e != hipSuccess ? hipGetErrorString(e) : "error word set (a hand-off wait timed out)");
    printf("LSTM CHECK FAILED: stopped at the first launch error\n"); fflush(stdout); exit(1);
  }
}
// runs the case on the device into p's outputs; false (with why) if it was not launched or a guard changed
static bool device_fwd(Fwd& p, const char* kernel, const char* what, char* why, size_t nwhy) {
  const int H = p.H, B = p.B, T = p.T;
  if (!resident(p.form == PLAIN ? SEQ_KIND_FWD_PLAIN : p.form == FUSED ? SEQ_KIND_FWD_FUSED : SEQ_KIND_FWD_OBS, H, seq_grid(H, B), why, nwhy)) return false;
  arena.reset();
  std::vector<float> g0 = p.form == PLAIN ? p.Gin : std::vector<float>((size_t)T * B * 4 * H, QNAN), hm((size_t)(T + 1) * p.bh(), QNAN), cm = hm, out((size_t)T * p.bh(), QNAN);
  std::copy(p.H0.begin(), p.H0.end(), hm.begin()); std::copy(p.C0.begin(), p.C0.end(), cm.begin());
  const Win<float> G = arena.put(g0, true), Hm = arena.put(hm, true), Cm = arena.put(cm, true), Hout = arena.put(out, true), TanhC = arena.put(out, true), Whh = arena.put(p.Whh, false), keep = arena.put(p.keep, false);
  SeqFwdArgs a{};
  a.G = G.d; a.Whh = Whh.d; a.Hm = Hm.d; a.Cm = Cm.d; a.Hout = Hout.d; a.TanhC = TanhC.d; a.keep = keep.d;
  a.counters = sync_words; a.err = sync_words + 256; a.T = T; a.B = B; a.stamps = nullptr; a.timeout_ticks = timeout_ticks;
  if (p.form != PLAIN) {
    a.X = arena.put(p.X, false).d; a.Wih = arena.put(p.Wih, false).d; a.bias = arena.put(p.bias, false).d;
    if (p.form == OBS) { a.ldx = a.ldw = p.ld; a.kx = p.kx; }
  }
  prepare_launch();
  if (!seq_fwd_launch(0, H, a, 0)) { snprintf(why, nwhy, "no kernel for this hidden size"); return false; }
  finish_launch(kernel, what);
  bool ok = arena.get(G, p.G); ok = arena.get(Hm, p.Hm) && ok; ok = arena.get(Cm, p.Cm) && ok; ok = arena.get(Hout, p.Hout) && ok; ok = arena.get(TanhC, p.TanhC) && ok;
  if (!ok) snprintf(why, nwhy, "stray store (guard changed)");
  return ok;
}
static bool device_step(Fwd& p, const char* kernel, const char* what, char* why, size_t nwhy) {
  const int H = p.H;
  arena.reset();
  const Win<float> Hin = arena.put(p.H0, true), C = arena.put(p.C0, true), Hout = arena.put(std::vector<float>(p.bh(), QNAN), true);   // Hin between output guards too: it must come back unchanged
  StepArgs a{};
  a.X = arena.put(p.X, false).d; a.ldx = p.ld; a.kx = p.form == OBS ? p.kx : 0;
  a.Wih = arena.put(p.Wih, false).d; a.ldw = p.ld; a.Whh = arena.put(p.Whh, false).d; a.bias = arena.put(p.bias, false).d;
  a.Hin = Hin.d; a.Hout = Hout.d; a.C = C.d; a.M = p.B;
  prepare_launch();
  if (!lstm_step_launch(0, H, a)) { snprintf(why, nwhy, "no kernel for this hidden size"); return false; }
  finish_launch(kernel, what);
  std::vector<float> hin, c;
  bool ok = arena.get(Hin, hin); ok = arena.get(C, c) && ok; ok = arena.get(Hout, p.Hout) && ok;
  p.Hm.assign(2 * p.bh(), QNAN); p.Cm = p.Hm;
  std::copy(hin.begin(), hin.end(), p.Hm.begin()); std::copy(c.begin(), c.end(), p.Cm.begin() + p.bh());
  if (!ok) snprintf(why, nwhy, "stray store (guard changed)");
  return ok;
}
static bool device_bwd(Bwd& q, const char* kernel, const char* what, char* why, size_t nwhy) {
  const int H = q.H, B = q.B, T = q.T; const bool t16 = q.rows == BWD16_ROWS;
  if (!resident(t16 ? SEQ_KIND_BWD16 : SEQ_KIND_BWD32, H, t16 ? seq_bwd16_grid(H, B) : seq_grid(H, B), why, nwhy)) return false;
  arena.reset();
  const Win<float> dG = arena.put(std::vector<float>((size_t)T * B * 4 * H, QNAN), true), db = arena.put(q.db0, true), part = arena.put(std::vector<float>((size_t)q.nrg() * 4 * H, QNAN), true);
  SeqBwdArgs a{};
  a.Gact = arena.put(q.Gact, false).d; a.TanhC = arena.put(q.TanhC, false).d; a.Cm = arena.put(q.Cm, false).d; a.dHabove = arena.put(q.dHa, false).d;
  a.keep = arena.put(q.keep, false).d; a.Whh = arena.put(q.Whh, false).d; a.dG = dG.d;
  a.counters = sync_words; a.err = sync_words + 256; a.T = T; a.B = B;
  a.db = db.d; a.db_part = q.part ? part.d : nullptr; a.timeout_ticks = timeout_ticks; a.stamps = nullptr;
  prepare_launch();
  if (!(t16 ? seq_bwd16_launch(0, H, a, 0) : seq_bwd_launch(0, H, a))) { snprintf(why, nwhy, "no kernel for this hidden size"); return false; }
  finish_launch(kernel, what);
  bool ok = arena.get(dG, q.dG); ok = arena.get(db, q.db) && ok; ok = arena.get(part, q.db_part) && ok;
  if (q.part) for (int j = 0; j < 4 * H; ++j) ok = ok && same_bits(q.db[j], q.db0[j]);   // deterministic mode leaves db to the ordered second stage
  if (!ok) snprintf(why, nwhy, "stray store (guard or, in deterministic mode, db changed)");
  return ok;
}

// ---- driver ------------------------------------------------------------------------------------------------------------------------------
static double worst_frac[8][NCAT], worst_free[8], worst_tanh_u = 0;   // per kernel name
static std::vector<std::string> kernel_names;
static int kernel_index(const char* k) { for (size_t i = 0; i < kernel_names.size(); ++i) if (kernel_names[i] == k) return (int)i; kernel_names.push_back(k); return (int)kernel_names.size() - 1; }

static std::string fractions(const Chk& k) {
  std::string s; char b[48];
  for (int c = 0; c < NCAT; ++c) if (k.seen[c]) { snprintf(b, sizeof b, " %s %.3f", CATN[c], k.worst[c]); s += b; }
  return s;
}
static void report_device(const char* kernel, const char* what, bool ran, const Chk& k, const char* why, double free_err) {
  const bool ok = ran && k.max_ratio() <= 1.0;
  const int ki = kernel_index(kernel);
  if (ran) { for (int c = 0; c < NCAT; ++c) worst_frac[ki][c] = std::max(worst_frac[ki][c], k.worst[c]); worst_tanh_u = std::max(worst_tanh_u, k.tanh_pure_u); }
  char fr[40] = ""; if (free_err >= 0) { snprintf(fr, sizeof fr, " free %.3g", free_err); worst_free[ki] = std::max(worst_free[ki], free_err); }
  printf("case %-10s %-40s : %s%s%s\n", kernel, what, ok ? "ok" : "FAIL ", ok ? fractions(k).c_str() : (ran ? k.why : why), ok ? fr : "");
  tally.count(ok);
}
// plan mode: alive gates, model accepted, mutants rejected
template <class P, class Model, class Check>
static void report_plan(const char* kernel, const char* what, int fam, P& prob, double alive, Model model, Check check, int T, int keep, int B, bool kx_short, bool part) {
  std::string line; char b[200]; bool ok = true;
  snprintf(b, sizeof b, "alive %.3f", alive); line += b;
  if (!(alive >= 0.9)) { ok = false; line += " FAIL fewer than 90% of the gate pre-activations within |x| <= 3;"; }
  model(prob, M_NONE);
  const Chk k0 = check(prob);
  if (k0.max_ratio() <= 1.0) line += " model ok"; else { ok = false; snprintf(b, sizeof b, " model FAIL (%s);", k0.why); line += b; }
  for (int i = 0; FAM_MUTS[fam][i]; ++i) {
    const int m = FAM_MUTS[fam][i];
    if (!exercised(fam, m, T, keep, B, kx_short, part)) { line += std::string(" ") + MUTN[m] + "=n/a"; continue; }
    model(prob, m);
    early_exit = true; rejected = false;
    const double r = check(prob).max_ratio();
    early_exit = false; rejected = false;
    if (r > 100.0) line += std::string(" ") + MUTN[m] + "=rejected";
    else { ok = false; snprintf(b, sizeof b, " %s=FAIL (passes within %.3g x bound)", MUTN[m], r); line += b; }
  }
  printf("case %-10s %-40s : %s %s\n", kernel, what, ok ? "planned" : "FAIL", line.c_str());
  tally.count(ok);
}

static uint32_t next_id = 1;
static void fwd_case(int form, int H, int B, int T, int kx, int keep) {
  static const char* KN[3] = {"fwd_plain", "fwd_fused", "fwd_obs"};
  char what[96];
  if (form == OBS) snprintf(what, sizeof what, "H=%d B=%d T=%d kx=%d keep=%s", H, B, T, kx, KEEPN[keep]);
  else snprintf(what, sizeof what, "H=%d B=%d T=%d keep=%s", H, B, T, KEEPN[keep]);
  Fwd p; make_fwd(p, H, B, T, form, kx, keep, next_id++);
  FwdRef ref; ref_fwd(p, ref);
  const bool kx_short = p.kx < p.KX;
  if (tally.plan_mode) { report_plan(KN[form], what, FAM_FWD, p, ref.alive, model_fwd, check_fwd, T, keep, B, kx_short, false); return; }
  char why[160] = "";
  const bool ran = device_fwd(p, KN[form], what, why, sizeof why);
  report_device(KN[form], what, ran, ran ? check_fwd(p) : Chk(), why, ran ? free_running_error(p, ref) : -1.0);
}
static void fwd_cases(int form, int H, int B, int T, int kx = 0) {
  if (T == 1) { fwd_case(form, H, B, T, kx, K_ONES); fwd_case(form, H, B, T, kx, K_ZEROS); }
  else for (int k = 0; k < NKEEP; ++k) fwd_case(form, H, B, T, kx, k);
}
static void bwd_case(int rows, int H, int B, int T, bool part, int keep) {
  const char* kernel = rows == BWD16_ROWS ? "bwd16" : (H <= SEQ_FUSED_MAX_H ? "bwd" : "bwd_wide");
  char what[96]; snprintf(what, sizeof what, "H=%d B=%d T=%d bias=%s keep=%s", H, B, T, part ? "part" : "atomic", KEEPN[keep]);
  Bwd q; const double alive = make_bwd(q, H, B, T, rows, part, keep, next_id++);
  if (tally.plan_mode) { report_plan(kernel, what, FAM_BWD, q, alive, model_bwd, check_bwd, T, keep, B, false, part); return; }
  char why[160] = "";
  const bool ran = device_bwd(q, kernel, what, why, sizeof why);
  report_device(kernel, what, ran, ran ? check_bwd(q) : Chk(), why, -1.0);
}
static void bwd_cases(int rows, int H, int B, int T) {
  for (int part = 0; part < 2; ++part) {
    if (T == 1) { bwd_case(rows, H, B, T, part, K_ONES); bwd_case(rows, H, B, T, part, K_ZEROS); }
    else for (int k = 0; k < NKEEP; ++k) bwd_case(rows, H, B, T, part, k);
  }
}
static void step_case(int H, int M, bool obs) {
  const char* kernel = obs ? "step_obs" : "step";
  char what[96];
  if (obs) snprintf(what, sizeof what, "H=%d M=%d kx=%d grid=%d", H, M, KBJ_NOBS_ACTOR, lstm_step_grid(H, M));
  else snprintf(what, sizeof what, "H=%d M=%d grid=%d", H, M, lstm_step_grid(H, M));
  Fwd p; make_fwd(p, H, M, 1, obs ? OBS : FUSED, obs ? KBJ_NOBS_ACTOR : 0, K_ONES, next_id++);
  FwdRef ref; ref_fwd(p, ref);
  if (tally.plan_mode) { report_plan(kernel, what, FAM_STEP, p, ref.alive, model_step, check_step, 1, K_ONES, M, obs, false); return; }
  char why[160] = "";
  const bool ran = device_step(p, kernel, what, why, sizeof why);
  report_device(kernel, what, ran, ran ? check_step(p) : Chk(), why, -1.0);
}

int main(int argc, char** argv) {
  tally.args(argc, argv);
  if (!tally.plan_mode) {
    int dev = 0, wall_khz = 0;
    CK(hipGetDevice(&dev));
    CK(hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || wall_khz <= 0) wall_khz = 100000;
    timeout_ticks = (unsigned)std::min<long long>(0xFFFFFFFFll, (long long)SEQ_TIMEOUT_MS * wall_khz);
    arena.init();
    CK(hipMalloc(reinterpret_cast<void**>(&sync_words), 257 * sizeof(unsigned)));
  }
  static const int T125[3] = {1, 2, 5};
  // forward, plain: every hidden size the library serves; small / full / three row groups; the remapped grid (nblk % 8 == 0)
  for (int H = 64; H <= SEQ_MAX_H; H += 64) fwd_cases(PLAIN, H, 33, 3);
  for (int H : {64, 256}) for (int B : {1, 32, 70}) for (int T : T125) fwd_cases(PLAIN, H, B, T);
  fwd_cases(PLAIN, 64, 128, 3); fwd_cases(PLAIN, 192, 100, 3);
  // forward, input projection fused (hidden-layer input) and gates from the observation rows
  for (int H = 64; H <= SEQ_FUSED_MAX_H; H += 64) for (int T : {1, 3}) fwd_cases(FUSED, H, 33, T);
  for (int H : {64, 256}) for (int B : {1, 70}) for (int T : {1, 3}) fwd_cases(FUSED, H, B, T);
  for (int H = 64; H <= SEQ_FUSED_MAX_H; H += 64) for (int kx : {KBJ_NOBS_ACTOR, KBJ_LD_ACTOR}) fwd_cases(OBS, H, 33, 3, kx);
  // backward, 32 x 32 tiles (capped-register kernel up to 256, wide above)
  for (int H = 64; H <= SEQ_MAX_H; H += 64) for (int T : T125) bwd_cases(SEQ_ROWS, H, 33, T);
  for (int H : {64, 256, 512}) for (int B : {1, 70}) for (int T : T125) bwd_cases(SEQ_ROWS, H, B, T);
  // backward, 16 x 64 tiles
  for (int H = 64; H <= SEQ_FUSED_MAX_H; H += 64) for (int B : {1, 15, 16, 17, 48}) for (int T : T125) bwd_cases(BWD16_ROWS, H, B, T);
  bwd_cases(BWD16_ROWS, 64, 128, 2); bwd_cases(BWD16_ROWS, 256, 32, 2);
  // step kernel: one row group per workgroup, then 34 row groups on 32 chunks and 130 on 128 (ragged last group)
  for (int H = 64; H <= SEQ_FUSED_MAX_H; H += 64) for (int obs = 0; obs < 2; ++obs) for (int M : {1, 33}) step_case(H, M, obs != 0);
  step_case(256, 1061, false); step_case(64, 4129, false);
  if (!tally.plan_mode) {
    for (size_t i = 0; i < kernel_names.size(); ++i) {
      printf("worst fraction of the bound, %-10s:", kernel_names[i].c_str());
      for (int c = 0; c < NCAT; ++c) if (worst_frac[i][c] > 0 || c == C_LINK) printf(" %s %.3f", CATN[c], worst_frac[i][c]);
      if (worst_free[i] > 0) printf("   free-running worst |Hout error| %.3g", worst_free[i]);
      printf("\n");
    }
    printf("seq_tanh worst observed error %.2f u (derived C_tanh = %.0f u, C_sig = %.0f u)\n", worst_tanh_u, C_TANH, C_SIG);
  }
  return tally.finish("LSTM");
}
