// Check of the kernels behind the last LSTM layer of the rollout (kbj_nn_kernels.h) and of the two threefry streams that live there:
// actor_head_fused_kernel, critic_value_fused_kernel, carry_reset_kernel, lstm_cell_fwd_kernel, actor_head_lpf_kernel, init_uniform_kernel.
//   make -C tools head_check && tools/head_check            (GPU; ends with HEAD CHECK PASSED or a non-zero exit status)
//   tools/head_check --plan                                  (no device: the same case table; proves what the checker accepts and rejects)
// Every launch goes through the launch helpers of kbj_nn_kernels.h, the ones kbj_nn.hip calls: grids and blocks are under test with the kernels.
//
// u = 2^-24, gamma_n = n u / (1 - n u) (kbj_check.h). Every bound below is x SECOND_ORDER; a NaN fails.
//
// ACTOR HEAD. Every case runs twice from identical inputs, argmax = 1 then argmax = 0. Per (env n, joint j), in double from the kernel's inputs:
//   projection  P = h_n . W_row, S = sum |terms|:  e_P = (gamma_{H+2} + (H + 2) 2^-52) S    (the contraction bound as gemm_check forms it)
//   mean = P_j + bout_j + joint_bias_j + cmd:      e_mu = e_P + 3 u (|P| + |bout| + |bias| + |cmd|)         (three additions)
//   os = P_{20+j} + bout_{20+j}:                   e_os = e_P + u (|P| + |bout|)                             (one addition)
//   sp = softplus(os) = log1p(exp(os)) (os > 20: os; the two agree to 2e-9 there):  e_sp = e_os + 6 u sigmoid(os) + 4 u sp
//        (|softplus'| = sigmoid <= 1; expf within 3 ulp = 6 u relative, which log1p' = 1 / (1 + e) turns into 6 u sigmoid; log1pf within 2 ulp
//        = 4 u of its result: the OpenCL 3.0 section 7.4 maxima that the device library is built to)
//   sd = min((sp + min_std) var_scale, max_std):   e_sd = var_scale e_sp + 2 u (sp + min_std) var_scale       (a sum and a product; min is 1-Lipschitz)
//   y = y0 + alpha (mean - y0) (the new lpf):      e_y = alpha (e_mu + u |mean - y0|) + u |alpha (mean - y0)| + u |y|   (difference, product, sum)
//   log-prob term t_j = -z'^2 / 2 - log sd - log(2 pi) / 2 with z' = (a - y) / sd from the STORED action and lpf:
//        e_z' = |z'| (e_sd / (sd - e_sd) + 2 u)                                                                (difference and quotient)
//        e_t = |z'| e_z' + e_z'^2 + e_sd / (sd - e_sd) + 6 u |log sd| + 4 u (z'^2 / 2 + |log sd| + log(2 pi) / 2)   (logf within 3 ulp; four operations)
//   logp = sum_j t_j:                              sum e_t + gamma_20 sum |t_j|
//   the draw: z_ref from the exact integer threefry words (u1, u2 are exact in fp32), radius and cosine in double (of the fp32 product's
//        exact value c u2, c = 6.2831855f). (a - y) / sd_ref against z_ref within |z_ref| e_sd / (sd - e_sd) + (2 u |sd z| + u |a| + u |a - y|) / sd + E_Z.
//   Bit for bit: lpf after the sampled run == lpf after the argmax run; argmax action == stored lpf; rows {0, 17, 99} of an N = 100 case
//   relaunched as N = 1 with env_off + row give the same action, logp and lpf (the kernel's comment promises launch-shape independence).
// PURE DRAW (Wout = 0, lpf = 0, bout_j = -joint_bias_j, command columns 0, bout_{20+j} = 30 > 20: mean = 0 and sd = min(15.005, 1) = 1, all
//   exactly). The stored action IS the device's z: |a - z_ref| <= E_Z. With log 1 = 0 the terms are fp32 arithmetic of stored values, so logp is
//   demanded BIT FOR BIT as the fixed-order fp32 sum over j = 0..19 of fl(fl(-0.5 a_j a_j) - fl(0.5 log 2 pi)) (a fused -0.5 a a - 0 is the same
//   number). This is where "logp is the fixed-order sum of its own 20 terms" is exact; elsewhere the terms hold logf(sd) and are bounded above.
// E_Z, the one bound that cannot simply be asserted: E_Z = max(floor, 4 x worst |host fp32 restatement - z_ref| over the case's draws).
//   floor: the argument rounding of c u2 alone moves z by r |sin| u theta <= sqrt(2 x 24 ln 2) x 2 pi x u = 2.16e-6 (u1 >= 2^-24). The second part
//   stands for the device's logf / sqrtf / cosf (each within a few ulp where the host's are within one). A wrong key, counter word, joint or env
//   is O(1): the bound is not delicate. The worst observed fraction is printed at the end of a device run.
// CRITIC VALUE: h_n . w + b against double within (gamma_{H+2} + (H + 2) 2^-52) (S + |b|); rows {0, 17, 99} of N = 100 relaunched alone, bit for bit.
// CARRY RESET: exact. Rows whose done word compares != 0 (so -0.0 is NOT a reset) are +0 in every plane and in lpf; every other word keeps its bits.
// CELL FORWARD (c_out aliases c_prev, as the library calls it): gates against sigmoid / tanh of the fp32 pre-activation within C_sig u / C_tanh u
//   (the forms and constants of lstm_check: no contraction in front here); c against f c_prev + i g of the stored gates within 3 u (|f c| + |i g|);
//   with the masked outputs: tanhc within C_tanh u + 3 u (...), h == fl(o tanhc), hm == fl(h keep), cm == fl(c keep) BIT FOR BIT; without: h against
//   o tanh(c stored) within C_tanh u + u |h|.
// LOW-PASS-ONLY HEAD: the new lpf within e_y, with e_mu = 2 u (|out| + |bias| + |cmd|); columns 20..39 of `out` are NaN: they must not be read.
// INIT: bit for bit against the host (threefry is integer arithmetic, the scaling one exact product and one fmaf).
//
// HARNESS (kbj_check.h): every array a window, NaN around inputs, the pattern around outputs (the in-place lpf, action, logp, value, the carry
// planes and G among them); pure outputs start as NaN; the padding columns 65.. of the observation rows are NaN. Any HIP error ends the run at once.
//
// --plan (no device), over the same table: (1) the std entries on the max_std clamp are 10 % .. 90 % of a case's, some softplus arguments lie
// above 20 and some below -20; (2) the host draws over 2^20+ (env, step, joint) triples have mean 0, variance 1 and no lag-1 correlation along
// env, step or joint, each at 5 sigma of its sampling error (`case draws`, also part of a device run); (3) the checker passes a host fp32 model
// of every kernel; (4) it rejects every mutant of that model by more than 100 x the bound in every case that exercises it (`exercised`,
// mirrored by tests/test_gpu_head_check.py); other cases say n/a.
#include <functional>
#include "kbj_check.h"
#include "kbj_nn_kernels.h"

using namespace kbj;

constexpr double C_SIG = 4.0, C_TANH = 9.0, SECOND_ORDER = 1.01;   // C_SIG, C_TANH: derived in tools/lstm_check.hip for the same rcp / exp forms
static const double Z_FLOOR = std::sqrt(2.0 * 24.0 * std::log(2.0)) * 6.283185307179586 * U;   // 2.16e-6
static const float TWO_PI_F = 6.283185307179586f, HALF_LOG2PI_F = 0.5f * 1.8378770664093453f;
static inline float rnd(float x) { volatile float v = x; return v; }   // one fp32 rounding, never fused with its neighbour

static void fill(std::vector<float>& v, size_t n, uint32_t tag, float scale) { v.resize(n); for (size_t i = 0; i < n; ++i) v[i] = scale * val_real(hash3(tag, (uint32_t)(i >> 16), (uint32_t)(i & 0xFFFF))); }
static void dot(const float* x, const float* w, int n, double& s, double& a) { for (int k = 0; k < n; ++k) { const double p = (double)x[k] * w[k]; s += p; a += std::fabs(p); } }
static float dotf(const float* x, const float* w, int n) { float s = 0; for (int k = 0; k < n; ++k) s += x[k] * w[k]; return s; }
static double contraction(int H) { return gamma_n(H + 2) + (H + 2) * std::ldexp(1.0, -52); }

// threefry2x32-20 on the host (integer arithmetic: exact), and the two streams' draws from it
static inline uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static void threefry(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t& o0, uint32_t& o1) {
  static const int rot[8] = {13, 15, 26, 6, 17, 29, 16, 24};
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  uint32_t x0 = c0 + ks[0], x1 = c1 + ks[1];
  for (int g = 0; g < 5; ++g) {
    for (int r = 0; r < 4; ++r) { x0 += x1; x1 = rotl(x1, rot[(g & 1) * 4 + r]); x1 ^= x0; }
    x0 += ks[(g + 1) % 3]; x1 += ks[(g + 2) % 3] + (uint32_t)(g + 1);
  }
  o0 = x0; o1 = x1;
}
static inline uint32_t action_key(uint32_t seed) { return seed ^ ((uint32_t)KBJ_RNG_ACTION * 0x9E3779B9u); }
static double z_double(uint32_t b0, uint32_t b1) {
  const float u1 = (float)((b0 >> 8) + 1u) * (1.0f / 16777216.0f), u2 = (float)(b1 >> 8) * (1.0f / 16777216.0f);
  return std::sqrt(-2.0 * std::log((double)u1)) * std::cos((double)TWO_PI_F * (double)u2);
}
static float z_float(uint32_t b0, uint32_t b1, bool plus1 = true) {
  const float u1 = (float)((b0 >> 8) + (plus1 ? 1u : 0u)) * (1.0f / 16777216.0f), u2 = (float)(b1 >> 8) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(TWO_PI_F * u2);
}

// ---- mutants ---------------------------------------------------------------------------------------------------------------------------
enum Mut { M_NONE = 0, M_ENV_OFF, M_TILE_ENV, M_CTR_SWAP, M_U1, M_STD_COL, M_CMD_COL, M_CLAMP, M_LPF_OP, M_LOGP19, M_LEAF, M_NEGZERO, NMUT };
static const char* MUTN[NMUT] = {"", "env_off_ignored", "tile_local_env", "counter_swapped", "u1_without_plus1", "std_from_column_j", "cmd_column_off_by_one",
                                 "clamp_before_var_scale", "lpf_wrong_operand", "logp_19_joints", "leaf_ignored", "negzero_is_done"};
enum Family { FAM_ACTOR, FAM_PURE, FAM_LPF, FAM_INIT, FAM_CARRY, FAM_NONE };
static const int FAM_MUTS[6][10] = {{M_ENV_OFF, M_TILE_ENV, M_CTR_SWAP, M_U1, M_STD_COL, M_CMD_COL, M_CLAMP, M_LPF_OP, M_LOGP19, 0},
                                    {M_ENV_OFF, M_TILE_ENV, M_CTR_SWAP, M_U1, M_STD_COL, M_CMD_COL, M_CLAMP, M_LPF_OP, M_LOGP19, 0},
                                    {M_CMD_COL, M_LPF_OP, 0}, {M_LEAF, 0}, {M_NEGZERO, 0}, {0}};
struct Traits { int N = 0; uint32_t env_off = 0, leaf = 0; bool tail = false, hashed_done = false; };
// does a case exercise what the mutant breaks? (a rule on the case's parameters)
static bool exercised(int fam, int mut, const Traits& t) {
  switch (mut) {
    case M_ENV_OFF: return t.env_off != 0;
    case M_TILE_ENV: return t.N > HEAD_ENVS;          // the second tile's rows are the first whose tile-local index differs
    case M_U1: return t.tail;                          // only a draw with a tiny u1 tells (k + 1) / 2^24 from k / 2^24 by more than the bound
    case M_LPF_OP: return fam != FAM_PURE;            // mean = y0 = 0 there
    case M_LEAF: return t.leaf != 0;
    case M_NEGZERO: return t.hashed_done;             // the hashed pattern pins done[0] = -0.0
    default: return true;
  }
}

// ---- the checker's bookkeeping -----------------------------------------------------------------------------------------------------------
enum Cat { C_LPF = 0, C_Z, C_LOGP, C_LINK, C_SHAPE, C_VALUE, C_EXACT, C_GATE, C_CELL, C_TANHC, C_H, NCAT };
static const char* CATN[NCAT] = {"lpf", "z", "logp", "links", "relaunch", "value", "exact", "act", "c", "tanhc", "h"};
struct Chk {
  double worst[NCAT]; bool seen[NCAT]; char why[160];
  Chk() { for (int i = 0; i < NCAT; ++i) { worst[i] = 0; seen[i] = false; } why[0] = 0; }
  void upd(int cat, double err, double bound, long r, long c) {   // a NaN fails; exact checks pass err = 0 or infinity with bound = 0
    const double ratio = err == 0.0 ? 0.0 : (err <= bound ? err / bound : (bound > 0 && err == err ? err / bound : INFINITY));
    seen[cat] = true;
    if (ratio > worst[cat]) {
      if (ratio > 1.0 && max_ratio() <= 1.0) snprintf(why, sizeof why, "%s row=%ld col=%ld err %.3g bound %.3g", CATN[cat], r, c, err, bound);
      worst[cat] = ratio;
    }
  }
  void exact(int cat, float got, float want, long r, long c) { upd(cat, same_bits(got, want) ? 0.0 : INFINITY, 0.0, r, c); }
  void fail(int cat, const char* what) { seen[cat] = true; if (max_ratio() <= 1.0) snprintf(why, sizeof why, "%s", what); worst[cat] = INFINITY; }
  double max_ratio() const { double m = 0; for (int i = 0; i < NCAT; ++i) m = std::max(m, worst[i]); return m; }
};

static Arena arena((size_t)64 << 20);
static void finish_launch(const char* kernel, const char* what) {   // any HIP error ends the run: nothing further is launched
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    printf("case %-10s %-52s : FAIL %s\n", kernel, what, hipGetErrorString(e));
    printf("HEAD CHECK FAILED: stopped at the first launch error\n"); fflush(stdout); exit(1);
  }
}
static const char* cur_kernel = ""; static const char* cur_what = "";

// ---- actor head ------------------------------------------------------------------------------------------------------------------------
struct Head {
  int N = 0, H = 0, ld = KBJ_LD_ACTOR; uint32_t env_off = 0, step = 0, seed = 0; HeadParams hp{}; bool pure = false;
  std::vector<float> hin, Wout, bout, obs, lpf0, jb;               // inputs
  std::vector<float> lpf[2], act[2], logp[2];                       // outputs: [0] the argmax run, [1] the sampled run
  std::vector<int> sub_rows; std::vector<Head> subs;                // single rows relaunched as N = 1
  double e_z = 0, clamp_share = 0; int sp_hi = 0, sp_lo = 0;
};
static HeadParams default_hp(int ld) { return HeadParams{0.01f, 1.0f, 0.5f, 0.02f / (0.02f + 1.0f / (6.2831853f * 10.0f)), ld}; }
static double softplus_inv(double y) { return std::log(std::expm1(y)); }
static void head_draw_bound(Head& p) {
  double worst = 0;
  for (int n = 0; n < p.N; ++n) for (int j = 0; j < KBJ_NU; ++j) {
    uint32_t b0, b1; threefry(action_key(p.seed), p.env_off + (uint32_t)n, p.step, (uint32_t)j, b0, b1);
    worst = std::max(worst, std::fabs((double)z_float(b0, b1) - z_double(b0, b1)));
  }
  p.e_z = std::max(Z_FLOOR, 4.0 * worst);
}
static Head head_row(const Head& p, int r) {
  Head q; q.N = 1; q.H = p.H; q.ld = p.ld; q.env_off = p.env_off + (uint32_t)r; q.step = p.step; q.seed = p.seed; q.hp = p.hp; q.pure = p.pure;
  q.hin.assign(p.hin.begin() + (size_t)r * p.H, p.hin.begin() + (size_t)(r + 1) * p.H); q.Wout = p.Wout; q.bout = p.bout; q.jb = p.jb;
  q.obs.assign(p.obs.begin() + (size_t)r * p.ld, p.obs.begin() + (size_t)(r + 1) * p.ld);
  q.lpf0.assign(p.lpf0.begin() + (size_t)r * KBJ_NU, p.lpf0.begin() + (size_t)(r + 1) * KBJ_NU);
  q.e_z = p.e_z;
  return q;
}
static void make_head(Head& p, int H, int N, int ld, uint32_t env_off, uint32_t step, HeadParams hp, bool pure, uint32_t seed, uint32_t id) {
  p.N = N; p.H = H; p.ld = ld; p.env_off = env_off; p.step = step; p.hp = hp; p.hp.ld_obs = ld; p.pure = pure; p.seed = seed;
  const uint32_t tag = 0x48000000u + id * 16u;
  fill(p.hin, (size_t)N * H, tag + 1, 1.0f); fill(p.Wout, (size_t)2 * KBJ_NU * H, tag + 2, 1.0f / std::sqrt((float)H));
  fill(p.bout, 2 * KBJ_NU, tag + 3, 0.5f); fill(p.obs, (size_t)N * ld, tag + 4, 1.0f); fill(p.lpf0, (size_t)N * KBJ_NU, tag + 5, 1.0f); fill(p.jb, KBJ_NU, tag + 6, 0.5f);
  for (int n = 0; n < N; ++n) for (int c = KBJ_NOBS_ACTOR; c < ld; ++c) p.obs[(size_t)n * ld + c] = QNAN;
  if (pure) {
    std::fill(p.Wout.begin(), p.Wout.end(), 0.0f); std::fill(p.lpf0.begin(), p.lpf0.end(), 0.0f);
    for (int j = 0; j < KBJ_NU; ++j) { p.bout[j] = -p.jb[j]; p.bout[KBJ_NU + j] = 30.0f; }
    for (int n = 0; n < N; ++n) for (int c = 0; c < 10; ++c) p.obs[(size_t)n * ld + KBJ_OBS_CMD + 6 + c] = 0.0f;
  } else {
    // std biases spread by +-1 around the pre-activation at which (softplus + min_std) var_scale meets max_std; joint 18 far above 20, joint 19 far below -20
    const float centre = (float)softplus_inv((double)hp.max_std / hp.var_scale - hp.min_std);
    for (int j = 0; j < KBJ_NU; ++j) p.bout[KBJ_NU + j] = centre + 2.0f * p.bout[KBJ_NU + j];
    p.bout[KBJ_NU + 18] = 25.0f; p.bout[KBJ_NU + 19] = -25.0f;
  }
  head_draw_bound(p);
  long on = 0;
  for (int n = 0; n < N; ++n) for (int j = 0; j < KBJ_NU; ++j) {
    double s = p.bout[KBJ_NU + j], a = 0; dot(&p.hin[(size_t)n * H], &p.Wout[(size_t)(KBJ_NU + j) * H], H, s, a);
    p.sp_hi += s > 20.0; p.sp_lo += s < -20.0;
    on += ((s > 20.0 ? s : std::log1p(std::exp(s))) + hp.min_std) * hp.var_scale >= hp.max_std;
  }
  p.clamp_share = (double)on / ((double)N * KBJ_NU);
  if (N == 100) { p.sub_rows = {0, 17, 99}; for (int r : p.sub_rows) p.subs.push_back(head_row(p, r)); }
}
// host fp32 model of actor_head_fused_kernel from its source comments, and its mutants
static void model_head(Head& p, int mut) {
  const int N = p.N, H = p.H; const HeadParams& hp = p.hp;
  for (int run = 0; run < 2; ++run) {
    p.lpf[run] = p.lpf0; p.act[run].assign((size_t)N * KBJ_NU, QNAN); p.logp[run].assign(N, QNAN);
    for (int n = 0; n < N; ++n) {
      float lps[KBJ_NU];
      for (int j = 0; j < KBJ_NU; ++j) {
        const float om = dotf(&p.hin[(size_t)n * H], &p.Wout[(size_t)j * H], H) + p.bout[j];
        const float os = mut == M_STD_COL ? om : dotf(&p.hin[(size_t)n * H], &p.Wout[(size_t)(KBJ_NU + j) * H], H) + p.bout[KBJ_NU + j];
        const float mean = om + p.jb[j] + (j >= 10 ? p.obs[(size_t)n * p.ld + KBJ_OBS_CMD + 6 + (j - 10) - (mut == M_CMD_COL ? 1 : 0)] : 0.0f);
        const float sp = os > 20.0f ? os : log1pf(expf(os));
        const float sd = mut == M_CLAMP ? fminf(sp + hp.min_std, hp.max_std) * hp.var_scale : fminf((sp + hp.min_std) * hp.var_scale, hp.max_std);
        const float y0 = p.lpf0[(size_t)n * KBJ_NU + j];
        const float y = mut == M_LPF_OP ? mean + hp.alpha * (y0 - mean) : y0 + hp.alpha * (mean - y0);
        p.lpf[run][(size_t)n * KBJ_NU + j] = y;
        float a = y;
        if (run == 1) {
          uint32_t b0, b1;
          const uint32_t env = (mut == M_ENV_OFF ? 0u : p.env_off) + (uint32_t)(mut == M_TILE_ENV ? n % HEAD_ENVS : n);
          if (mut == M_CTR_SWAP) threefry(action_key(p.seed), env, (uint32_t)j, p.step, b0, b1); else threefry(action_key(p.seed), env, p.step, (uint32_t)j, b0, b1);
          a = y + sd * z_float(b0, b1, mut != M_U1);
        }
        p.act[run][(size_t)n * KBJ_NU + j] = a;
        const float z = (a - y) / sd;
        lps[j] = -0.5f * z * z - logf(sd) - HALF_LOG2PI_F;
      }
      p.logp[run][n] = chain(lps, mut == M_LOGP19 ? KBJ_NU - 1 : KBJ_NU, 1);
    }
  }
  for (Head& q : p.subs) model_head(q, mut);
}
static bool device_head(Head& p, char* why, size_t nwhy) {
  bool ok = true;
  for (int run = 0; run < 2; ++run) {
    arena.reset();
    const Win<float> lpf = arena.put(p.lpf0, true), act = arena.put(std::vector<float>((size_t)p.N * KBJ_NU, QNAN), true), logp = arena.put(std::vector<float>(p.N, QNAN), true);
    const float* hin = arena.put(p.hin, false).d; const float* W = arena.put(p.Wout, false).d; const float* b = arena.put(p.bout, false).d;
    const float* obs = arena.put(p.obs, false).d; const float* jb = arena.put(p.jb, false).d;
    actor_head_fused_launch(0, hin, p.H, W, b, obs, lpf.d, jb, p.hp, p.seed, p.env_off, p.step, run == 0, p.N, act.d, logp.d);
    finish_launch(cur_kernel, cur_what);
    ok = arena.get(lpf, p.lpf[run]) && ok; ok = arena.get(act, p.act[run]) && ok; ok = arena.get(logp, p.logp[run]) && ok;
  }
  for (Head& q : p.subs) ok = device_head(q, why, nwhy) && ok;
  if (!ok) snprintf(why, nwhy, "stray store (guard changed)");
  return ok;
}
static Chk check_head(const Head& p) {
  Chk k;
  const int N = p.N, H = p.H; const HeadParams& hp = p.hp;
  const double gc = contraction(H), half_log2pi = 0.5 * std::log(2.0 * 3.14159265358979323846);
  for (int n = 0; n < N; ++n) {
    double et_sum[2] = {0, 0}, t_abs[2] = {0, 0}, t_sum[2] = {0, 0};
    for (int j = 0; j < KBJ_NU; ++j) {
      const size_t i = (size_t)n * KBJ_NU + j;
      double pm = 0, sm = 0, ps = 0, ss = 0;
      dot(&p.hin[(size_t)n * H], &p.Wout[(size_t)j * H], H, pm, sm); dot(&p.hin[(size_t)n * H], &p.Wout[(size_t)(KBJ_NU + j) * H], H, ps, ss);
      const double cmd = j >= 10 ? p.obs[(size_t)n * p.ld + KBJ_OBS_CMD + 6 + (j - 10)] : 0.0;
      const double mean = pm + p.bout[j] + p.jb[j] + cmd, e_mu = gc * sm + 3 * U * (std::fabs(pm) + std::fabs(p.bout[j]) + std::fabs(p.jb[j]) + std::fabs(cmd));
      const double os = ps + p.bout[KBJ_NU + j], e_os = gc * ss + U * (std::fabs(ps) + std::fabs(p.bout[KBJ_NU + j]));
      const double sp = os > 40.0 ? os : std::log1p(std::exp(os)), e_sp = e_os + 6 * U / (1.0 + std::exp(-os)) + 4 * U * sp;
      const double sd = std::min((sp + hp.min_std) * (double)hp.var_scale, (double)hp.max_std), e_sd = hp.var_scale * e_sp + 2 * U * (sp + hp.min_std) * hp.var_scale;
      const double y0 = p.lpf0[i], y = y0 + hp.alpha * (mean - y0);
      const double e_y = hp.alpha * (e_mu + U * std::fabs(mean - y0)) + U * std::fabs(hp.alpha * (mean - y0)) + U * std::fabs(y);
      const double rel_sd = e_sd / (sd - e_sd);
      for (int run = 0; run < 2; ++run) {
        const float ys = p.lpf[run][i], a = p.act[run][i];
        k.upd(C_LPF, std::fabs(ys - y), SECOND_ORDER * e_y, n, j);
        if (run == 0) k.exact(C_LINK, a, ys, n, j);                        // the mode is the filtered mean itself
        else k.exact(C_LINK, ys, p.lpf[0][i], n, 100 + j);                  // sampling does not touch the low-pass state
        const double d = (double)a - (double)ys, zq = d / sd;
        if (run == 1) {
          uint32_t b0, b1; threefry(action_key(p.seed), p.env_off + (uint32_t)n, p.step, (uint32_t)j, b0, b1);
          const double zr = z_double(b0, b1);
          k.upd(C_Z, std::fabs(zq - zr), SECOND_ORDER * (std::fabs(zr) * rel_sd + (2 * U * std::fabs(sd * zr) + U * std::fabs(a) + U * std::fabs(d)) / sd + p.e_z), n, j);
          if (p.pure) k.upd(C_Z, std::fabs((double)a - zr), p.e_z, n, j);   // the stored action is the device's z itself: E_Z alone
        }
        const double lsd = std::log(sd), t = -0.5 * zq * zq - lsd - half_log2pi, e_zq = std::fabs(zq) * (rel_sd + 2 * U);
        et_sum[run] += std::fabs(zq) * e_zq + e_zq * e_zq + rel_sd + 6 * U * std::fabs(lsd) + 4 * U * (0.5 * zq * zq + std::fabs(lsd) + half_log2pi);
        t_sum[run] += t; t_abs[run] += std::fabs(t);
      }
    }
    for (int run = 0; run < 2; ++run) {
      k.upd(C_LOGP, std::fabs(p.logp[run][n] - t_sum[run]), SECOND_ORDER * (et_sum[run] + gamma_n(KBJ_NU) * t_abs[run]), n, run);
      if (p.pure) {   // mean 0, sd 1: the action is the draw and the terms are fp32 arithmetic of stored values
        float lps[KBJ_NU];
        for (int j = 0; j < KBJ_NU; ++j) { const float a = p.act[run][(size_t)n * KBJ_NU + j]; lps[j] = rnd(rnd(rnd(-0.5f * a) * a) - HALF_LOG2PI_F); }
        k.exact(C_LINK, p.logp[run][n], chain(lps, KBJ_NU, 1), n, 200 + run);
      }
    }
  }
  for (size_t s = 0; s < p.subs.size(); ++s) {
    const Head& q = p.subs[s]; const int r = p.sub_rows[s];
    if (q.act[0].size() != KBJ_NU) { k.fail(C_SHAPE, "single-row relaunch missing"); continue; }
    for (int run = 0; run < 2; ++run) {
      for (int j = 0; j < KBJ_NU; ++j) { k.exact(C_SHAPE, q.act[run][j], p.act[run][(size_t)r * KBJ_NU + j], r, j); k.exact(C_SHAPE, q.lpf[run][j], p.lpf[run][(size_t)r * KBJ_NU + j], r, 100 + j); }
      k.exact(C_SHAPE, q.logp[run][0], p.logp[run][r], r, 200);
    }
  }
  return k;
}

// ---- critic value ------------------------------------------------------------------------------------------------------------------------
struct Critic { int N = 0, H = 0; std::vector<float> hin, w, b, value; std::vector<int> sub_rows; std::vector<Critic> subs; };
static void make_critic(Critic& p, int H, int N, uint32_t id) {
  p.N = N; p.H = H; const uint32_t tag = 0x43000000u + id * 16u;
  fill(p.hin, (size_t)N * H, tag + 1, 1.0f); fill(p.w, H, tag + 2, 1.0f / std::sqrt((float)H)); fill(p.b, 1, tag + 3, 0.5f);
  if (N == 100) { p.sub_rows = {0, 17, 99}; for (int r : p.sub_rows) { Critic q; q.N = 1; q.H = H; q.w = p.w; q.b = p.b; q.hin.assign(p.hin.begin() + (size_t)r * H, p.hin.begin() + (size_t)(r + 1) * H); p.subs.push_back(q); } }
}
static void model_critic(Critic& p, int) { p.value.resize(p.N); for (int n = 0; n < p.N; ++n) p.value[n] = dotf(&p.hin[(size_t)n * p.H], p.w.data(), p.H) + p.b[0]; for (Critic& q : p.subs) model_critic(q, 0); }
static bool device_critic(Critic& p, char* why, size_t nwhy) {
  arena.reset();
  const Win<float> v = arena.put(std::vector<float>(p.N, QNAN), true);
  critic_value_fused_launch(0, arena.put(p.hin, false).d, p.H, arena.put(p.w, false).d, arena.put(p.b, false).d, p.N, v.d);
  finish_launch(cur_kernel, cur_what);
  bool ok = arena.get(v, p.value);
  for (Critic& q : p.subs) ok = device_critic(q, why, nwhy) && ok;
  if (!ok) snprintf(why, nwhy, "stray store (guard changed)");
  return ok;
}
static Chk check_critic(const Critic& p) {
  Chk k;
  for (int n = 0; n < p.N; ++n) { double s = p.b[0], a = std::fabs(s); dot(&p.hin[(size_t)n * p.H], p.w.data(), p.H, s, a); k.upd(C_VALUE, std::fabs(p.value[n] - s), contraction(p.H) * a, n, 0); }
  for (size_t s = 0; s < p.subs.size(); ++s) k.exact(C_SHAPE, p.subs[s].value[0], p.value[p.sub_rows[s]], p.sub_rows[s], 0);
  return k;
}

// ---- carry reset -------------------------------------------------------------------------------------------------------------------------
enum DonePat { D_NONE = 0, D_ALL, D_HASH };
static const char* DONEN[3] = {"none", "all", "hashed"};
struct Carry { int cnt = 0, H = 0, np = 0, stride = 1, pat = 0; bool has_lpf = false; std::vector<float> done, lpf0, lpf; std::vector<std::vector<float>> planes0, planes; };
static void make_carry(Carry& p, int cnt, int H, int np, bool has_lpf, int stride, int pat, uint32_t id) {
  p.cnt = cnt; p.H = H; p.np = np; p.has_lpf = has_lpf; p.stride = stride; p.pat = pat; const uint32_t tag = 0x52000000u + id * 16u;
  fill(p.done, (size_t)cnt * stride, tag, 1.0f);   // the other columns of a strided record: anything but the flag
  for (int r = 0; r < cnt; ++r) {
    static const float V[5] = {0.0f, 0.0f, -1.0f, 1.0f, -0.0f};
    p.done[(size_t)r * stride] = pat == D_NONE ? 0.0f : pat == D_ALL ? (r & 1 ? 1.0f : -1.0f) : V[hash3(tag + 1, r, 0) % 5u];
  }
  if (pat == D_HASH) { p.done[0] = -0.0f; if (cnt > 1) p.done[(size_t)stride] = -1.0f; if (cnt > 2) p.done[(size_t)2 * stride] = 0.0f; }
  p.planes0.resize(np); for (int q = 0; q < np; ++q) fill(p.planes0[q], (size_t)cnt * H, tag + 2 + q, 1.0f);
  fill(p.lpf0, (size_t)cnt * KBJ_NU, tag + 12, 1.0f);
}
static void model_carry(Carry& p, int mut) {
  p.planes = p.planes0; p.lpf = p.lpf0;
  for (int r = 0; r < p.cnt; ++r) {
    const float d = p.done[(size_t)r * p.stride]; uint32_t bits; memcpy(&bits, &d, 4);
    if (!(mut == M_NEGZERO ? bits != 0 : d != 0.0f)) continue;
    for (auto& pl : p.planes) std::fill(pl.begin() + (size_t)r * p.H, pl.begin() + (size_t)(r + 1) * p.H, 0.0f);
    if (p.has_lpf) std::fill(p.lpf.begin() + (size_t)r * KBJ_NU, p.lpf.begin() + (size_t)(r + 1) * KBJ_NU, 0.0f);
  }
}
static bool device_carry(Carry& p, char* why, size_t nwhy) {
  arena.reset();
  CarryPlanes cp{}; cp.n = p.np;
  std::vector<Win<float>> w(p.np);
  for (int q = 0; q < p.np; ++q) { w[q] = arena.put(p.planes0[q], true); cp.p[q] = w[q].d; }
  const Win<float> lpf = arena.put(p.lpf0, true);
  carry_reset_launch(0, cp, p.cnt, p.H, p.has_lpf ? lpf.d : nullptr, arena.put(p.done, false).d, p.stride);
  finish_launch(cur_kernel, cur_what);
  bool ok = arena.get(lpf, p.lpf); p.planes.resize(p.np);
  for (int q = 0; q < p.np; ++q) ok = arena.get(w[q], p.planes[q]) && ok;
  if (!ok) snprintf(why, nwhy, "stray store (guard changed)");
  return ok;
}
static Chk check_carry(const Carry& p) {
  Chk k;
  for (int r = 0; r < p.cnt; ++r) {
    const bool reset = p.done[(size_t)r * p.stride] != 0.0f;
    for (int q = 0; q < p.np; ++q) for (int u = 0; u < p.H; ++u) { const size_t i = (size_t)r * p.H + u; k.exact(C_EXACT, p.planes[q][i], reset ? 0.0f : p.planes0[q][i], r, q * 1000 + u); }
    for (int j = 0; j < KBJ_NU; ++j) { const size_t i = (size_t)r * KBJ_NU + j; k.exact(C_EXACT, p.lpf[i], reset && p.has_lpf ? 0.0f : p.lpf0[i], r, -1 - j); }
  }
  return k;
}

// ---- cell forward --------------------------------------------------------------------------------------------------------------------------
struct Cell { int M = 0, H = 0; bool masked = false; std::vector<float> G0, c0, keep, G, h, c, hm, cm, tc; };
static void make_cell(Cell& p, int M, int H, bool masked, uint32_t id) {
  p.M = M; p.H = H; p.masked = masked; const uint32_t tag = 0x4C000000u + id * 16u;
  fill(p.G0, (size_t)M * 4 * H, tag + 1, 3.0f); fill(p.c0, (size_t)M * H, tag + 2, 1.0f);
  p.keep.resize(M); for (int m = 0; m < M; ++m) p.keep[m] = hash3(tag + 3, m, 0) % 10u < 3u ? 0.0f : 1.0f;
  if (M > 1) { p.keep[0] = 0.0f; p.keep[1] = 1.0f; }
}
static float h_sig(float x) { return 1.0f / (1.0f + expf(-x)); }
static float h_tanh(float x) { return 1.0f - 2.0f / (1.0f + expf(2.0f * x)); }
static void model_cell(Cell& p, int) {
  const int H = p.H; const size_t mh = (size_t)p.M * H;
  p.G = p.G0; p.c = p.c0; p.h.assign(mh, QNAN); p.hm.assign(mh, QNAN); p.cm = p.hm; p.tc = p.hm;
  for (int m = 0; m < p.M; ++m) for (int u = 0; u < H; ++u) {
    float* g = &p.G[(size_t)m * 4 * H]; const size_t i = (size_t)m * H + u;
    const float ig = h_sig(g[u]), fg = h_sig(g[H + u]), gg = h_tanh(g[2 * H + u]), og = h_sig(g[3 * H + u]);
    const float c = fg * p.c0[i] + ig * gg, tc = h_tanh(c), h = og * tc;
    g[u] = ig; g[H + u] = fg; g[2 * H + u] = gg; g[3 * H + u] = og; p.h[i] = h; p.c[i] = c;
    if (p.masked) { p.hm[i] = h * p.keep[m]; p.cm[i] = c * p.keep[m]; p.tc[i] = tc; }
  }
}
static bool device_cell(Cell& p, char* why, size_t nwhy) {
  arena.reset();
  const size_t mh = (size_t)p.M * p.H; const std::vector<float> nanv(mh, QNAN);
  const Win<float> G = arena.put(p.G0, true), c = arena.put(p.c0, true), h = arena.put(nanv, true), hm = arena.put(nanv, true), cm = arena.put(nanv, true), tc = arena.put(nanv, true);
  CellFwdArgs2 ca{};
  ca.a[0] = CellFwdArgs{G.d, c.d, h.d, c.d, p.masked ? hm.d : nullptr, p.masked ? cm.d : nullptr, p.masked ? tc.d : nullptr, p.masked ? arena.put(p.keep, false).d : nullptr, p.M, p.H};
  lstm_cell_fwd_launch(0, ca, 1);
  finish_launch(cur_kernel, cur_what);
  bool ok = arena.get(G, p.G); ok = arena.get(c, p.c) && ok; ok = arena.get(h, p.h) && ok; ok = arena.get(hm, p.hm) && ok; ok = arena.get(cm, p.cm) && ok; ok = arena.get(tc, p.tc) && ok;
  if (!ok) snprintf(why, nwhy, "stray store (guard changed)");
  return ok;
}
static Chk check_cell(const Cell& p) {
  Chk k; const int H = p.H;
  for (int m = 0; m < p.M; ++m) for (int u = 0; u < H; ++u) {
    const size_t i = (size_t)m * H + u; const float* g = &p.G[(size_t)m * 4 * H]; const float* g0 = &p.G0[(size_t)m * 4 * H];
    for (int gate = 0; gate < 4; ++gate) {
      const double x = g0[gate * H + u], ref = gate == 2 ? std::tanh(x) : 1.0 / (1.0 + std::exp(-x));
      k.upd(C_GATE, std::fabs(g[gate * H + u] - ref), (gate == 2 ? C_TANH : C_SIG) * U, m, gate * 1000 + u);
    }
    const double ig = g[u], fg = g[H + u], gg = g[2 * H + u], og = g[3 * H + u], c = fg * p.c0[i] + ig * gg, mag = std::fabs(fg * p.c0[i]) + std::fabs(ig * gg);
    k.upd(C_CELL, std::fabs(p.c[i] - c), 3 * U * mag, m, u);
    if (p.masked) {
      k.upd(C_TANHC, std::fabs(p.tc[i] - std::tanh(c)), C_TANH * U + 3 * U * mag, m, u);
      k.exact(C_LINK, p.h[i], rnd((float)og * p.tc[i]), m, u);
      k.exact(C_LINK, p.hm[i], rnd(p.h[i] * p.keep[m]), m, 1000 + u); k.exact(C_LINK, p.cm[i], rnd(p.c[i] * p.keep[m]), m, 2000 + u);
    } else {
      const double h = og * std::tanh((double)p.c[i]);
      k.upd(C_H, std::fabs(p.h[i] - h), SECOND_ORDER * (C_TANH * U + U * std::fabs(h)), m, u);
      if (!(p.hm[i] != p.hm[i] && p.cm[i] != p.cm[i] && p.tc[i] != p.tc[i])) k.fail(C_LINK, "a masked output was written without being asked for");
    }
  }
  return k;
}

// ---- low-pass-only head ------------------------------------------------------------------------------------------------------------------
struct Lpf { int N = 0, ld = KBJ_LD_ACTOR; float alpha = 0; std::vector<float> out, obs, jb, lpf0, lpf; };
static void make_lpf(Lpf& p, int N, int ld, uint32_t id) {
  p.N = N; p.ld = ld; p.alpha = default_hp(ld).alpha; const uint32_t tag = 0x46000000u + id * 16u;
  fill(p.out, (size_t)N * 40, tag + 1, 1.0f); fill(p.obs, (size_t)N * ld, tag + 2, 1.0f); fill(p.jb, KBJ_NU, tag + 3, 0.5f); fill(p.lpf0, (size_t)N * KBJ_NU, tag + 4, 1.0f);
  for (int n = 0; n < N; ++n) { for (int c = KBJ_NU; c < 40; ++c) p.out[(size_t)n * 40 + c] = QNAN; for (int c = KBJ_NOBS_ACTOR; c < ld; ++c) p.obs[(size_t)n * ld + c] = QNAN; }
}
static void model_lpf(Lpf& p, int mut) {
  p.lpf = p.lpf0;
  for (int n = 0; n < p.N; ++n) for (int j = 0; j < KBJ_NU; ++j) {
    const float mean = p.out[(size_t)n * 40 + j] + p.jb[j] + (j >= 10 ? p.obs[(size_t)n * p.ld + KBJ_OBS_CMD + 6 + (j - 10) - (mut == M_CMD_COL ? 1 : 0)] : 0.0f);
    const float y0 = p.lpf0[(size_t)n * KBJ_NU + j];
    p.lpf[(size_t)n * KBJ_NU + j] = mut == M_LPF_OP ? mean + p.alpha * (y0 - mean) : y0 + p.alpha * (mean - y0);
  }
}
static bool device_lpf(Lpf& p, char* why, size_t nwhy) {
  arena.reset();
  const Win<float> lpf = arena.put(p.lpf0, true);
  actor_head_lpf_launch(0, arena.put(p.out, false).d, arena.put(p.obs, false).d, lpf.d, arena.put(p.jb, false).d, p.alpha, p.N, p.ld);
  finish_launch(cur_kernel, cur_what);
  const bool ok = arena.get(lpf, p.lpf);
  if (!ok) snprintf(why, nwhy, "stray store (guard changed)");
  return ok;
}
static Chk check_lpf(const Lpf& p) {
  Chk k;
  for (int n = 0; n < p.N; ++n) for (int j = 0; j < KBJ_NU; ++j) {
    const size_t i = (size_t)n * KBJ_NU + j;
    const double o = p.out[(size_t)n * 40 + j], cmd = j >= 10 ? p.obs[(size_t)n * p.ld + KBJ_OBS_CMD + 6 + (j - 10)] : 0.0, mean = o + p.jb[j] + cmd;
    const double e_mu = 2 * U * (std::fabs(o) + std::fabs(p.jb[j]) + std::fabs(cmd)), y0 = p.lpf0[i], y = y0 + p.alpha * (mean - y0);
    k.upd(C_LPF, std::fabs(p.lpf[i] - y), SECOND_ORDER * (p.alpha * (e_mu + U * std::fabs(mean - y0)) + U * std::fabs(p.alpha * (mean - y0)) + U * std::fabs(y)), n, j);
  }
  return k;
}

// ---- init ----------------------------------------------------------------------------------------------------------------------------------
struct Init { size_t n = 0; uint32_t leaf = 0, seed = 0; float bound = 0; std::vector<float> p; };
static float init_value(uint32_t seed, uint32_t leaf, size_t i, float bound) {
  uint32_t b0, b1; threefry(seed ^ ((uint32_t)KBJ_RNG_INIT * 0x9E3779B9u), leaf, (uint32_t)((uint64_t)i >> 32), (uint32_t)i, b0, b1);
  return fmaf(2 * bound, (float)(b0 >> 8) * (1.0f / 16777216.0f), -bound);
}
static void model_init(Init& q, int mut) { q.p.resize(q.n); for (size_t i = 0; i < q.n; ++i) q.p[i] = init_value(q.seed, mut == M_LEAF ? 0u : q.leaf, i, q.bound); }
static bool device_init(Init& q, char* why, size_t nwhy) {
  arena.reset();
  const Win<float> p = arena.put(std::vector<float>(q.n, QNAN), true);
  init_uniform_launch(0, p.d, q.n, q.bound, q.seed, q.leaf);
  finish_launch(cur_kernel, cur_what);
  const bool ok = arena.get(p, q.p);
  if (!ok) snprintf(why, nwhy, "stray store (guard changed)");
  return ok;
}
static Chk check_init(const Init& q) { Chk k; for (size_t i = 0; i < q.n; ++i) k.exact(C_EXACT, q.p[i], init_value(q.seed, q.leaf, i, q.bound), (long)i, 0); return k; }

// ---- driver ------------------------------------------------------------------------------------------------------------------------------
static double worst_frac[8][NCAT];
static std::vector<std::string> kernel_names;
static int kernel_index(const char* k) { for (size_t i = 0; i < kernel_names.size(); ++i) if (kernel_names[i] == k) return (int)i; kernel_names.push_back(k); return (int)kernel_names.size() - 1; }
static std::string fractions(const Chk& k) {
  std::string s; char b[48];
  for (int c = 0; c < NCAT; ++c) if (k.seen[c]) { snprintf(b, sizeof b, " %s %.3f", CATN[c], k.worst[c]); s += b; }
  return s;
}
// one case: on the device, or (plan mode) the model accepted and every mutant rejected where exercised; `live` / `live_ok`: the liveness figures of the inputs
template <class P>
static void run_case(const char* kernel, const char* what, int fam, const Traits& tr, P& prob, const std::function<void(P&, int)>& model,
                     const std::function<bool(P&, char*, size_t)>& device, const std::function<Chk(const P&)>& check, const std::string& live = "", bool live_ok = true) {
  cur_kernel = kernel; cur_what = what;
  if (!tally.plan_mode) {
    char why[160] = "";
    const bool ran = device(prob, why, sizeof why);
    const Chk k = ran ? check(prob) : Chk();
    const bool ok = ran && live_ok && k.max_ratio() <= 1.0;
    if (ran) for (int c = 0; c < NCAT; ++c) worst_frac[kernel_index(kernel)][c] = std::max(worst_frac[kernel_index(kernel)][c], k.worst[c]);
    printf("case %-10s %-52s : %s%s%s\n", kernel, what, ok ? "ok" : "FAIL ", ok ? fractions(k).c_str() : (ran ? (k.max_ratio() > 1.0 ? k.why : "inputs not live") : why), ok ? live.c_str() : "");
    tally.count(ok);
    return;
  }
  std::string line = live; char b[200]; bool ok = live_ok;
  if (!live_ok) line += " FAIL inputs not live;";
  model(prob, M_NONE);
  const Chk k0 = check(prob);
  if (k0.max_ratio() <= 1.0) line += " model ok"; else { ok = false; snprintf(b, sizeof b, " model FAIL (%s);", k0.why); line += b; }
  for (int i = 0; FAM_MUTS[fam][i]; ++i) {
    const int m = FAM_MUTS[fam][i];
    if (!exercised(fam, m, tr)) { line += std::string(" ") + MUTN[m] + "=n/a"; continue; }
    model(prob, m);
    const double r = check(prob).max_ratio();
    if (r > 100.0) line += std::string(" ") + MUTN[m] + "=rejected";
    else { ok = false; snprintf(b, sizeof b, " %s=FAIL (passes within %.3g x bound)", MUTN[m], r); line += b; }
  }
  printf("case %-10s %-52s : %s%s\n", kernel, what, ok ? "planned" : "FAIL", line.c_str());
  tally.count(ok);
}

static uint32_t next_id = 1;
static double worst_pure_z = 0, worst_e_z = 0;
static void actor_case(int H, int N, int ld, uint32_t off, uint32_t step, const char* hpn, HeadParams hp) {
  char what[96]; snprintf(what, sizeof what, "H=%d N=%d ld=%d off=%u step=%u hp=%s", H, N, ld, off, step, hpn);
  Head p; make_head(p, H, N, ld, off, step, hp, false, 0xC0FFEE11u + next_id, next_id); ++next_id;
  char live[96]; snprintf(live, sizeof live, " clamp %.3f sp_hi %d sp_lo %d", p.clamp_share, p.sp_hi, p.sp_lo);
  Traits tr; tr.N = N; tr.env_off = off;
  run_case<Head>("actor", what, FAM_ACTOR, tr, p, model_head, device_head, check_head, live, p.clamp_share >= 0.1 && p.clamp_share <= 0.9 && p.sp_hi > 0 && p.sp_lo > 0);
  worst_e_z = std::max(worst_e_z, p.e_z);
}
// the smallest seed counter whose case holds a draw with u1 < 2^-18 and |cos| >= 1/2: the one place that tells (k + 1) 2^-24 from k 2^-24
static uint32_t tail_seed(int N, uint32_t off, uint32_t step) {
  for (uint32_t s = 1;; ++s) {
    const uint32_t seed = mix(s);
    for (int n = 0; n < N; ++n) for (int j = 0; j < KBJ_NU; ++j) {
      uint32_t b0, b1; threefry(action_key(seed), off + (uint32_t)n, step, (uint32_t)j, b0, b1);
      if ((b0 >> 8) < 64u && std::fabs(std::cos(6.283185307179586 * (double)(b1 >> 8) / 16777216.0)) >= 0.5) return seed;
    }
  }
}
static void pure_case(int N, uint32_t off, uint32_t step, bool tail) {
  char what[96]; snprintf(what, sizeof what, "H=64 N=%d off=%u step=%u seed=%s", N, off, step, tail ? "tail" : "fixed");
  Head p; make_head(p, 64, N, KBJ_LD_ACTOR, off, step, default_hp(KBJ_LD_ACTOR), true, tail ? tail_seed(N, off, step) : 0x5EED0000u + next_id, next_id); ++next_id;
  Traits tr; tr.N = N; tr.env_off = off; tr.tail = tail;
  char live[96]; snprintf(live, sizeof live, " e_z %.3g", p.e_z);
  run_case<Head>("actor_pure", what, FAM_PURE, tr, p, model_head, device_head, check_head, live);
  worst_e_z = std::max(worst_e_z, p.e_z);
  if (!tally.plan_mode && !p.act[1].empty()) for (int n = 0; n < N; ++n) for (int j = 0; j < KBJ_NU; ++j) {
    uint32_t b0, b1; threefry(action_key(p.seed), off + (uint32_t)n, step, (uint32_t)j, b0, b1);
    const double e = std::fabs(p.act[1][(size_t)n * KBJ_NU + j] - z_double(b0, b1)); if (e == e) worst_pure_z = std::max(worst_pure_z, e);
  }
}
// mean, variance and the lag-1 correlations along env, step and joint of the host draws, each at 5 sigma of its sampling error
static void draws_case() {
  const int NE = 256, NS = 205, NJ = KBJ_NU; const uint32_t off = 1000, seed = 0xD1CE5EEDu;
  std::vector<double> z((size_t)NE * NS * NJ);
  for (int e = 0; e < NE; ++e) for (int s = 0; s < NS; ++s) for (int j = 0; j < NJ; ++j) { uint32_t b0, b1; threefry(action_key(seed), off + e, s, j, b0, b1); z[((size_t)e * NS + s) * NJ + j] = z_double(b0, b1); }
  const double n = (double)z.size();
  double m = 0, v = 0; for (double x : z) m += x; m /= n; for (double x : z) v += (x - m) * (x - m); v /= n;
  auto lag = [&](int de, int ds, int dj) {   // correlation of neighbours along one axis; second: the number of pairs
    double c = 0, cnt = 0;
    for (int e = 0; e + de < NE; ++e) for (int s = 0; s + ds < NS; ++s) for (int j = 0; j + dj < NJ; ++j) {
      c += (z[((size_t)e * NS + s) * NJ + j] - m) * (z[((size_t)(e + de) * NS + s + ds) * NJ + j + dj] - m); cnt += 1;
    }
    return std::make_pair(c / cnt / v, cnt);
  };
  const auto re = lag(1, 0, 0), rs = lag(0, 1, 0), rj = lag(0, 0, 1);
  const bool ok = std::fabs(m) < 5 / std::sqrt(n) && std::fabs(v - 1) < 5 * std::sqrt(2 / n) && std::fabs(re.first) < 5 / std::sqrt(re.second) && std::fabs(rs.first) < 5 / std::sqrt(rs.second) && std::fabs(rj.first) < 5 / std::sqrt(rj.second);
  char what[96]; snprintf(what, sizeof what, "envs=%d steps=%d joints=%d off=%u", NE, NS, NJ, off);
  printf("case %-10s %-52s : %s triples %.0f mean %.2f var %.2f rho_env %.2f rho_step %.2f rho_joint %.2f (in sigma)\n", "draws", what, ok ? (tally.plan_mode ? "planned" : "ok") : "FAIL", n,
         m * std::sqrt(n), (v - 1) / std::sqrt(2 / n), re.first * std::sqrt(re.second), rs.first * std::sqrt(rs.second), rj.first * std::sqrt(rj.second));
  tally.count(ok);
}

int main(int argc, char** argv) {
  tally.args(argc, argv);
  if (!tally.plan_mode) arena.init();
  const HeadParams d68 = default_hp(KBJ_LD_ACTOR);
  // actor head: ragged tiles, ragged workgroups, several workgroups; every hidden size; both row strides; the key add wrapping inside the launch; the head's parameters
  for (int H : {64, 256}) for (int N : {1, 15, 16, 17, 63, 64, 65, 100, 130}) actor_case(H, N, KBJ_LD_ACTOR, 0, 0, "default", d68);
  for (int H = 64; H <= 512; H += 64) actor_case(H, 33, KBJ_LD_ACTOR, 0, 0, "default", d68);
  for (int N : {33, 100}) actor_case(64, N, KBJ_LD_OF(KBJ_NOBS_ACTOR + 4), 0, 0, "default", d68);
  for (uint32_t off : {1000u, 0xFFFFFFF0u}) for (uint32_t step : {5u, 0x80000007u}) for (int H : {64, 256}) actor_case(H, 100, KBJ_LD_ACTOR, off, step, "default", d68);
  { HeadParams h;
    h = d68; h.max_std = 0.35f; actor_case(64, 33, KBJ_LD_ACTOR, 1000, 5, "max_std=0.35", h);
    h = d68; h.min_std = 0.2f; actor_case(64, 33, KBJ_LD_ACTOR, 1000, 5, "min_std=0.2", h);
    h = d68; h.var_scale = 1.5f; actor_case(64, 33, KBJ_LD_ACTOR, 1000, 5, "var_scale=1.5", h);
    h = d68; h.var_scale = 0.25f; actor_case(64, 33, KBJ_LD_ACTOR, 1000, 5, "var_scale=0.25", h);
    h = d68; h.alpha = 1.0f; actor_case(64, 33, KBJ_LD_ACTOR, 1000, 5, "lpf_alpha=1", h);
    h = d68; h.alpha = 0.1f; actor_case(64, 33, KBJ_LD_ACTOR, 1000, 5, "lpf_alpha=0.1", h); }
  pure_case(100, 0, 0, false); pure_case(130, 1000, 5, false); pure_case(100, 0xFFFFFFF0u, 0x80000007u, false); pure_case(130, 1000, 5, true);
  draws_case();
  // critic value
  for (int N : {1, 7, 8, 9, 100}) for (int H = 64; H <= 512; H += 64) {
    char what[96]; snprintf(what, sizeof what, "H=%d N=%d", H, N);
    Critic p; make_critic(p, H, N, next_id++);
    run_case<Critic>("critic", what, FAM_NONE, Traits(), p, model_critic, device_critic, check_critic);
  }
  // carry reset
  for (int cnt : {1, 3, 4, 5, 130}) for (int H : {64, 192, 512}) for (int np : {2, 8}) for (int lpf = 1; lpf >= 0; --lpf) for (int stride : {1, (int)KBJ_AUX_SIZE}) for (int pat = 0; pat < 3; ++pat) {
    char what[96]; snprintf(what, sizeof what, "cnt=%d H=%d planes=%d lpf=%d stride=%d done=%s", cnt, H, np, lpf, stride, DONEN[pat]);
    Carry p; make_carry(p, cnt, H, np, lpf != 0, stride, pat, next_id++);
    Traits tr; tr.hashed_done = pat == D_HASH;
    run_case<Carry>("carry", what, FAM_CARRY, tr, p, model_carry, device_carry, check_carry);
  }
  // cell forward
  for (int M : {1, 33}) for (int H : {64, 256, 512}) for (int masked = 0; masked < 2; ++masked) {
    char what[96]; snprintf(what, sizeof what, "H=%d M=%d masked=%d", H, M, masked);
    Cell p; make_cell(p, M, H, masked != 0, next_id++);
    run_case<Cell>("cell", what, FAM_NONE, Traits(), p, model_cell, device_cell, check_cell);
  }
  // low-pass-only head
  for (int N : {1, 13, 100}) for (int ld : {(int)KBJ_LD_ACTOR, (int)KBJ_LD_OF(KBJ_NOBS_ACTOR + 4)}) {
    char what[96]; snprintf(what, sizeof what, "N=%d ld=%d", N, ld);
    Lpf p; make_lpf(p, N, ld, next_id++);
    run_case<Lpf>("lpf", what, FAM_LPF, Traits(), p, model_lpf, device_lpf, check_lpf);
  }
  // init
  for (size_t n : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)70001}) for (uint32_t leaf : {0u, 7u}) for (int bi = 0; bi < 2; ++bi) {
    Init q; q.n = n; q.leaf = leaf; q.seed = 0x1234ABCDu + next_id++; q.bound = bi ? 1.0f / std::sqrt(475.0f) : 0.125f;
    char what[96]; snprintf(what, sizeof what, "n=%zu leaf=%u bound=%s", n, leaf, bi ? "1/sqrt(475)" : "1/8");
    Traits tr; tr.leaf = leaf;
    run_case<Init>("init", what, FAM_INIT, tr, q, model_init, device_init, check_init);
  }
  if (!tally.plan_mode) {
    for (size_t i = 0; i < kernel_names.size(); ++i) {
      printf("worst fraction of the bound, %-10s:", kernel_names[i].c_str());
      for (int c = 0; c < NCAT; ++c) if (worst_frac[i][c] > 0 || c == C_LINK) printf(" %s %.3f", CATN[c], worst_frac[i][c]);
      printf("\n");
    }
    printf("pure draw: worst |z - z_ref| %.3g = %.3f of E_Z (largest E_Z of the table %.3g, floor %.3g)\n", worst_pure_z, worst_pure_z / worst_e_z, worst_e_z, Z_FLOOR);
  } else printf("largest E_Z of the table %.3g (floor %.3g)\n", worst_e_z, Z_FLOOR);
  return tally.finish("HEAD");
}
