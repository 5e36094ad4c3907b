// Check of what kbj_ppo_grad runs between the GEMMs and the recurrences (kbj_nn_kernels.h): the minibatch gathers and re-pitching kernels, the actor
// head over a minibatch trajectory (two parallel stages, two time scans, the Gaussian log-prob), the advantage statistics, ppo_loss_kernel,
// critic_head_kernel<VPL>, the mirror loss, the metrics line, the kernels of the folded input projection and the bias gradients, and sumsq_kernel.
//   make -C tools update_check && tools/update_check         (GPU; ends with UPDATE CHECK PASSED or a non-zero exit status)
//   tools/update_check --plan                                 (no device: the same case table; proves what the checker accepts and rejects)
// Every launch goes through the *_launch helpers of kbj_nn_kernels.h, the ones kbj_nn.hip calls: grids and blocks are under test with the kernels.
// One `Ops` object stands for "run this kernel on these host arrays": on the device (upload between guards, launch, download) or as a host fp32
// model of the kernel's source (plan mode, with mutants). Cases, links between launches and checks are written once, on top of it.
//
// u = 2^-24, gamma_n = n u / (1 - n u); u_d = 2^-53, gamma_d likewise. A product feeding a sum may or may not be contracted: every bound below
// holds for both forms, and bit-for-bit demands are made only where both sides run the same kernel code or the arithmetic is additions / copies.
// References are double precision from the STORED inputs of the stage under test; a NaN fails.
//
// A. GATHERS, RE-PITCHING: copies, bit for bit; destination padding and outputs outside the launched column range keep the pattern. mirror_rows:
//    mul in + add within u |mul in| + u |out| (one product, one sum); entries with mul = +-1, add = 0 bit for bit. The two tables are the ones
//    build_mirror_tables (kbj_nn_kernels.h, the function the library calls) makes from a model whose joint biases and ranges are hashed.
// B. ACTOR HEAD OVER A MINIBATCH (bounds written for inputs with errors e_x; a stage on its own has e_x = 0, the chained case propagates them):
//    pre:   y0 = out + bias + cmd: 2 u (|out| + |bias| + |cmd|). sd as in head_check: e_sp = 6 u sigmoid + 4 u sp (expf 3 ulp, log1pf 2 ulp),
//           e_sd = var_scale e_sp + 2 u (sp + min_std) var_scale; on the clamp sd == max_std bit for bit.
//    fwd:   y_t = s + alpha (m - s), s = y_{t-1} keep_{t-1} (from the device's own y_{t-1}): (1 - alpha) e_s + alpha e_m + alpha u |m - s| + u |alpha (m - s)| + u |y|.
//    logp:  z = (a - y) / sd: e_z = (e_y + u |a - y|) / sd + |z| rel_sd + u |z|; term -z^2/2 - log sd - c: |z| e_z + e_z^2 + rel_sd + 6 u |log sd| (logf 3 ulp)
//           + 4 u (z^2/2 + |log sd| + c); sum of 20: gamma_20 sum |terms|. entropy term 0.5 + c + log sd: rel_sd + 6 u |log sd| + 2 u (c + .5 + |log sd|).
//    bwd_pre: dmean = gl z / sd + dy: |gl| (e_z / sd + |z / sd| rel_sd) + 2 u |gl z / sd| + u (|gl z / sd| + |dy|).
//           gs = gl (z^2 - 1) / sd + dent / sd, dstd = gs var_scale sigmoid(raw): roundings counted in check_head; sigmoidf_ within C_SIG u (lstm_check);
//           exactly +0 on the clamp.
//    bwd:   gy = g + keep gc; out = alpha gy; gc = (1 - alpha) gy: e_gy = e_g + keep e_gc + u |gy|, e_out = alpha e_gy + u |out|, e_gc = (1 - alpha) e_gy + 2 u |gc|.
//    Links, bit for bit: a T-step forward launch == T one-step launches chained by the host through lpf0 = y keep (a reset passes +0); a backward launch
//    over the prefix [0, t0) == the first t0 steps of the T-step launch for rows with keep[t0 - 1] = 0, and a one-step launch == step t wherever keep[t] = 0
//    or t = T - 1 (the reverse scan's chunks are aligned to T - 1, so a SUFFIX launch shares its chunk boundaries with the full one and would prove
//    nothing about them: the prefix launch has other boundaries); rows {0, B/2, B-1} relaunched alone as B = 1.
// C. adv_stats / sumsq: double sums of exact products: gamma_d(count + 2) sum |terms|; deterministic form: every block's partial against the double sum of
//    exactly its elements, empty blocks +0.0, reduce_double over the device's partials == the host chain bit for bit, two launches the same bits.
//    ppo_loss (check_loss): a = (adv - mean) / (sd + eps): fp32 branch var carries 6 u (var + mean^2) (the kernel's own comment: 3 eps32 (1 + mean^2 / var)
//    relative), mean u |mean|; double branch one rounding. ratio = expf(clamped d): 6 u ratio + ratio u |d|. dlogp = -inv a ratio: inv (e_a ratio + |a| e_ratio)
//    + 3 u |dlogp|. value half: gv from one of (v - tg), (vcl - tg), 0: u-counted in value_ref; dvalue = vcoef inv gv: 3 u |dvalue| + vcoef inv e_gv.
//    critic_head: value within gamma_{2 VPL + 7} (sum |h w| + |b|) (VPL products and sums per lane, six shuffle additions, the bias); the loss from the
//    device's own value; dh == fl(dvalue w) and dout[.][0] == dvalue bit for bit, dout[.][1..39] untouched.
//    mirror_loss: e = y + ym (u), dy = 2 ca e with ca = sa / (20 R): 3 u |dy|; dvalue += gv, gv = 2 sc / R ev: 3 u |gv| + u |dvalue|.
//    metrics: the host's double expression rounded once: u |x| + 8 u_d sum |terms|.
// D. matvec: gamma_{2 ceil(K / 64) + 7}; matvec_t_acc: gamma_{2 ceil(K / 64) + 3} per partial row (+ 16 atomic additions and y in the atomic form);
//    outer_acc: u (2 |u v| + |C|); colsum partials: additions only, bit for bit against the kernel's order (four phase chains over m = ph + 4 by + 2048 j,
//    then ((p0 + p1) + p2) + p3); atomic form gamma_{ceil(M / 2048) + 3 + 512 + 1}.
//
// INPUTS. Hashed families. Loss and critic-head samples are drawn so that every discrete outcome is live (>= 5 % of a case with R >= 255) and no
// sample sits on a threshold: a sample whose decision quantity (ratio - (1 +- clip), |ratio - 1| - clip, |d| - lrclip, |dv| - vclip, |v - tg| - |vcl - tg|,
// a against 0; pre - max_std in group B) is within 8 x its fp32 error bound of the threshold is re-drawn with the next salt. --plan prints the
// re-draws and the number of remaining violations (0) per case; every sample is compared on the device.
// --plan also (2) proves that a balanced-tree sum of the same partials differs from the chain wherever an order is demanded, (3) passes the host
// fp32 model of every kernel through the same checker, (4) rejects every mutant by > 100 x the bound in every case that exercises it, n/a elsewhere.
#include <functional>
#include <map>
#include "kbj_check.h"
#include "kbj_nn_kernels.h"

using namespace kbj;

constexpr double C_SIG = 4.0, SECOND_ORDER = 1.01, MARGIN = 8.0;
static const double UD = std::ldexp(1.0, -53);
static inline double gamma_d(double n) { return n * UD / (1.0 - n * UD); }
static const float HALF_LOG2PI_F = 0.5f * kLog2Pi;
static const double HALF_LOG2PI = 0.5 * (double)kLog2Pi;
static inline float hv(uint32_t tag, size_t i, uint32_t salt = 0) { return val_real(hash3(tag + salt * 0x01000193u, (uint32_t)(i >> 16), (uint32_t)(i & 0xFFFF))); }
static inline float hu(uint32_t tag, size_t i, uint32_t salt = 0) { return 0.5f * (hv(tag, i, salt) + 1.0f); }   // [0, 1)
static void fill(std::vector<float>& v, size_t n, uint32_t tag, float scale, float off = 0.0f) { v.resize(n); for (size_t i = 0; i < n; ++i) v[i] = off + scale * hv(tag, i); }
static std::vector<float> pat(size_t n) { return std::vector<float>(n, PATTERN); }
static std::vector<double> patd(size_t n) { return std::vector<double>(n, pattern<double>()); }
static double softplus_inv(double y) { return std::log(std::expm1(y)); }

// ---- mutants -----------------------------------------------------------------------------------------------------------------------------
enum Mut { M_NONE = 0, M_CHUNK, M_KEEP_NEIGH, M_KEEP_BWD, M_ALPHA_SWAP, M_CMD_COL, M_STD_COL, M_CLAMP, M_CLAMP_DERIV, M_LOGP19, M_ENT_GS, M_PART, M_STATS11,
           M_FP32_200, M_CLIP_D, M_VZERO, M_VCOEF, M_INV, M_CH_BIAS, M_CH_DH, M_CH_DOUT, M_MIR_MAP, M_MIR_SIGN, M_IDX, M_TSTRIDE, M_CS_PHASE, M_CS_LD, M_SS_SCALE, NMUT };
static const char* MUTN[NMUT] = {"", "chunk_state_dropped", "keep_of_neighbour_step", "keep_ignored_in_bwd_carry", "alpha_swapped_in_bwd", "cmd_column_off_by_one",
                                 "std_from_column_j", "clamp_before_var_scale", "clamp_derivative_not_zeroed", "logp_19_joints", "entropy_dropped_from_gs", "part_mask_ignored",
                                 "stats11_ignored", "fp32_branch_at_200", "clip_test_on_d", "value_zero_branch_dropped", "vcoef_dropped", "inv_r_minus_1", "critic_bias_dropped",
                                 "critic_dh_neighbour_row", "critic_dout_column_1", "mirror_map_identity", "mirror_sign", "idx_ignored", "t_stride_b", "colsum_last_phase_dropped",
                                 "colsum_ld_as_n", "sumsq_without_scale"};
typedef std::vector<std::pair<int, bool>> Muts;   // (mutant, does the case exercise it)

// ---- the checker's bookkeeping -------------------------------------------------------------------------------------------------------------
struct Chk {
  std::map<std::string, double> worst; char why[200]; double mx = 0;
  Chk() { why[0] = 0; }
  void upd(const char* cat, double err, double bound, long r, long c) {   // a NaN fails; exact checks pass err = 0 or infinity with bound = 0
    const double ratio = err == 0.0 ? 0.0 : (err <= bound ? err / bound : (bound > 0 && err == err ? err / bound : INFINITY));
    double& w = worst[cat]; if (ratio > w) w = ratio;
    if (ratio > mx) { if (ratio > 1.0 && mx <= 1.0) snprintf(why, sizeof why, "%s row=%ld col=%ld err %.3g bound %.3g", cat, r, c, err, bound); mx = ratio; }
  }
  template <class T> void exact(const char* cat, T got, T want, long r, long c) { upd(cat, same_bits(got, want) ? 0.0 : INFINITY, 0.0, r, c); }
  void fail(const char* cat, const char* what) { worst[cat] = INFINITY; if (mx <= 1.0) snprintf(why, sizeof why, "%s: %s", cat, what); mx = INFINITY; }
  template <class T> void same(const char* cat, const std::vector<T>& got, const std::vector<T>& want) {
    if (got.size() != want.size()) { fail(cat, "size"); return; }
    for (size_t i = 0; i < got.size(); ++i) exact(cat, got[i], want[i], (long)i, 0);
  }
};

static Arena arena((size_t)192 << 20);
static const char* cur_kernel = ""; static const char* cur_what = "";
static void finish_launch() {   // any HIP error ends the run: nothing further is launched
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    printf("case %-12s %-60s : FAIL %s\n", cur_kernel, cur_what, hipGetErrorString(e));
    printf("UPDATE CHECK FAILED: stopped at the first launch error\n"); fflush(stdout); exit(1);
  }
}

struct HeadHp { HeadParams hp; };
struct SmallIO { std::vector<float> action, logp, value, adv, target, aux, action_o, logp_o, value_o, adv_o, target_o, keep_o; };

// ---- every kernel as an operation on host arrays: on the device, or the host fp32 model (with a mutant) --------------------------------------
struct Ops {
  bool dev = false; int mut = M_NONE; bool guards = true;
  template <class T> const T* in(const std::vector<T>& v) { return v.empty() ? nullptr : arena.put(v, false).d; }
  template <class T> Win<T> out(const std::vector<T>& v) { return v.empty() ? Win<T>() : arena.put(v, true); }
  template <class T> void back(const Win<T>& w, std::vector<T>& v) { if (w.d && !arena.get(w, v)) guards = false; }

  // -- group A
  void gather_rows(const std::vector<float>& src, const std::vector<int>& idx, int T, int N, int B, int wdt, int lds, int ldd, std::vector<float>& dst, bool misalign) {
    if (dev) {
      arena.reset();
      std::vector<float> s1; if (misalign) { s1.assign(1, QNAN); s1.insert(s1.end(), src.begin(), src.end()); }
      const float* s = misalign ? in(s1) + 1 : in(src); const Win<float> d = out(dst);
      gather_rows_launch(0, s, in(idx), T, N, B, wdt, lds, d.d, ldd); finish_launch(); back(d, dst); return;
    }
    for (int t = 0; t < T; ++t) for (int b = 0; b < B; ++b) for (int k = 0; k < wdt; ++k)
      dst[((size_t)t * B + b) * ldd + k] = src[((size_t)t * (mut == M_TSTRIDE ? B : N) + (mut == M_IDX ? b : idx[b])) * lds + k];
  }
  void gather_small(SmallIO& s, const std::vector<int>& idx, int T, int N, int B, int c0, int c1) {
    if (dev) {
      arena.reset();
      const Win<float> ao = out(s.action_o), lo = out(s.logp_o), vo = out(s.value_o), av = out(s.adv_o), to = out(s.target_o), ko = out(s.keep_o);
      GatherSmallArgs a{in(s.action), in(s.logp), in(s.value), in(s.adv), in(s.target), in(s.aux), ao.d, lo.d, vo.d, av.d, to.d, ko.d};
      gather_small_launch(0, a, in(idx), T, N, B, c0, c1); finish_launch();
      back(ao, s.action_o); back(lo, s.logp_o); back(vo, s.value_o); back(av, s.adv_o); back(to, s.target_o); back(ko, s.keep_o); return;
    }
    for (int t = 0; t < T; ++t) for (int b = 0; b < B; ++b) for (int c = c0; c < c1; ++c) {
      const size_t r = (size_t)t * B + b, src = (size_t)t * (mut == M_TSTRIDE ? B : N) + (mut == M_IDX ? b : idx[b]);
      if (c < KBJ_NU) s.action_o[r * KBJ_NU + c] = s.action[src * KBJ_NU + c];
      else if (c == KBJ_NU) { if (!s.logp.empty()) s.logp_o[r] = s.logp[src]; }
      else if (c == KBJ_NU + 1) { if (!s.value.empty()) s.value_o[r] = s.value[src]; }
      else if (c == KBJ_NU + 2) { if (!s.adv.empty()) s.adv_o[r] = s.adv[src]; }
      else if (c == KBJ_NU + 3) { if (!s.target.empty()) s.target_o[r] = s.target[src]; }
      else s.keep_o[r] = s.aux[src * KBJ_AUX_SIZE + KBJ_AUX_DONE] != 0 ? 0.0f : 1.0f;
    }
  }
  void gather_carry(const std::vector<std::vector<float>>& src, std::vector<std::vector<float>>& dst, int nplanes, int nlpf, const std::vector<int>& idx, int B, int H) {
    if (dev) {
      arena.reset();
      GatherCarryArgs a{}; a.nplanes = nplanes; a.nlpf = nlpf; std::vector<Win<float>> w(src.size());
      for (size_t p = 0; p < src.size(); ++p) { a.src[p] = in(src[p]); w[p] = out(dst[p]); a.dst[p] = w[p].d; }
      gather_carry_launch(0, a, in(idx), B, H); finish_launch();
      for (size_t p = 0; p < src.size(); ++p) back(w[p], dst[p]);
      return;
    }
    for (int p = 0; p < nplanes + nlpf; ++p) { const int w = p < nplanes ? H : KBJ_NU; for (int b = 0; b < B; ++b) for (int k = 0; k < w; ++k) dst[p][(size_t)b * w + k] = src[p][(size_t)(mut == M_IDX ? b : idx[b]) * w + k]; }
  }
  void mirror_rows(const std::vector<float>& x, std::vector<float>& y, size_t rows, int ld, const std::vector<MirrorEntry>& tab) {
    if (dev) {
      arena.reset();
      std::vector<MirrorEntry> img(tab.size() + 2 * GUARD, MirrorEntry{0, QNAN, QNAN}); std::copy(tab.begin(), tab.end(), img.begin() + GUARD);   // entries around the table read element 0 and give NaN
      MirrorEntry* t = reinterpret_cast<MirrorEntry*>(arena.take(img.size() * sizeof(MirrorEntry))); CK(hipMemcpy(t, img.data(), img.size() * sizeof(MirrorEntry), hipMemcpyHostToDevice));
      const Win<float> o = out(y); mirror_rows_launch(0, in(x), o.d, rows, ld, t + GUARD); finish_launch(); back(o, y); return;
    }
    for (size_t r = 0; r < rows; ++r) for (int k = 0; k < ld; ++k) y[r * ld + k] = tab[k].mul * x[r * ld + tab[k].src] + tab[k].add;
  }
  void repitch_rows(const std::vector<float>& src, int rows, int cols, int ld, std::vector<float>& dst) {
    if (dev) { arena.reset(); const Win<float> o = out(dst); repitch_rows_launch(0, in(src), rows, cols, ld, o.d); finish_launch(); back(o, dst); return; }
    for (int r = 0; r < rows; ++r) for (int c = 0; c < ld; ++c) dst[(size_t)r * ld + c] = c < cols ? src[(size_t)r * cols + c] : 0.0f;
  }
  void repitch_pad(const std::vector<float>& src, std::vector<float>& dst, size_t rows, int ws, int wd) {
    if (dev) { arena.reset(); const Win<float> o = out(dst); repitch_pad_launch(0, in(src), o.d, rows, ws, wd); finish_launch(); back(o, dst); return; }
    for (size_t r = 0; r < rows; ++r) for (int c = 0; c < wd; ++c) dst[r * wd + c] = c < ws ? src[r * ws + c] : 0.0f;
  }
  // -- group B
  void head_pre(const std::vector<float>& o, const std::vector<float>& obs, const std::vector<float>& jb, HeadParams hp, int R, std::vector<float>& y, std::vector<float>& sd) {
    if (dev) { arena.reset(); const Win<float> wy = out(y), ws = out(sd); actor_head_pre_launch(0, in(o), in(obs), in(jb), hp, R, wy.d, ws.d); finish_launch(); back(wy, y); back(ws, sd); return; }
    for (int r = 0; r < R; ++r) for (int j = 0; j < KBJ_NU; ++j) {
      y[(size_t)r * KBJ_NU + j] = o[(size_t)r * 40 + j] + jb[j] + (j >= 10 ? obs[(size_t)r * hp.ld_obs + KBJ_OBS_CMD + 6 + (j - 10) - (mut == M_CMD_COL ? 1 : 0)] : 0.0f);
      const float raw = o[(size_t)r * 40 + (mut == M_STD_COL ? 0 : KBJ_NU) + j], sp = raw > 20.0f ? raw : log1pf(expf(raw));
      sd[(size_t)r * KBJ_NU + j] = mut == M_CLAMP ? fminf(sp + hp.min_std, hp.max_std) * hp.var_scale : fminf((sp + hp.min_std) * hp.var_scale, hp.max_std);
    }
  }
  void train_fwd(const std::vector<float>& keep, const std::vector<float>& lpf0, HeadParams hp, int T, int B, std::vector<float>& y) {
    if (dev) { arena.reset(); const Win<float> wy = out(y); actor_head_train_fwd_launch(0, in(keep), in(lpf0), hp, T, B, wy.d); finish_launch(); back(wy, y); return; }
    for (int b = 0; b < B; ++b) for (int j = 0; j < KBJ_NU; ++j) {
      float state = lpf0[(size_t)b * KBJ_NU + j];
      for (int t = 0; t < T; ++t) {
        if (mut == M_CHUNK && t > 0 && t % 10 == 0) state = lpf0[(size_t)b * KBJ_NU + j];
        const size_t r = (size_t)t * B + b; const float yy = state + hp.alpha * (y[r * KBJ_NU + j] - state);
        y[r * KBJ_NU + j] = yy; state = yy * keep[mut == M_KEEP_NEIGH ? (size_t)std::min(t + 1, T - 1) * B + b : r];
      }
    }
  }
  void logp(const std::vector<float>& y, const std::vector<float>& sd, const std::vector<float>& act, int R, std::vector<float>& lp, std::vector<float>& en) {
    if (dev) { arena.reset(); const Win<float> wl = out(lp), we = out(en); gaussian_logp_launch(0, in(y), in(sd), in(act), R, wl.d, we.d); finish_launch(); back(wl, lp); back(we, en); return; }
    for (int r = 0; r < R; ++r) {
      float a = 0, e = 0;
      for (int j = 0; j < (mut == M_LOGP19 ? KBJ_NU - 1 : KBJ_NU); ++j) {
        const float s = sd[(size_t)r * KBJ_NU + j], z = (act[(size_t)r * KBJ_NU + j] - y[(size_t)r * KBJ_NU + j]) / s;
        a += -0.5f * z * z - logf(s) - HALF_LOG2PI_F; e += 0.5f + HALF_LOG2PI_F + logf(s);
      }
      lp[r] = a; en[r] = e;
    }
  }
  // act_is_y: the mirror form passes y itself as the action
  void bwd_pre(const std::vector<float>& o, const std::vector<float>& y, const std::vector<float>& sd, const std::vector<float>& act, bool act_is_y, const std::vector<float>& dlogp,
               const std::vector<float>& dy, float dent, HeadParams hp, int R, std::vector<float>& dout) {
    if (dev) {
      arena.reset(); const Win<float> wd = out(dout); const float* yd = in(y);
      actor_head_bwd_pre_launch(0, in(o), yd, in(sd), act_is_y ? yd : in(act), in(dlogp), in(dy), dent, hp, R, wd.d); finish_launch(); back(wd, dout); return;
    }
    for (int r = 0; r < R; ++r) for (int j = 0; j < KBJ_NU; ++j) {
      const size_t i = (size_t)r * KBJ_NU + j; const float s = sd[i], z = ((act_is_y ? y[i] : act[i]) - y[i]) / s, gl = dlogp[r];
      dout[(size_t)r * 40 + j] = gl * (z / s) + (dy.empty() ? 0.0f : dy[i]);
      const float gs = gl * ((z * z - 1.0f) / s) + (mut == M_ENT_GS ? 0.0f : dent / s), raw = o[(size_t)r * 40 + KBJ_NU + j];
      const float pre = ((raw > 20.0f ? raw : log1pf(expf(raw))) + hp.min_std) * hp.var_scale;
      dout[(size_t)r * 40 + KBJ_NU + j] = (pre < hp.max_std || mut == M_CLAMP_DERIV) ? gs * hp.var_scale * (1.0f / (1.0f + expf(-raw))) : 0.0f;
    }
  }
  void train_bwd(const std::vector<float>& keep, HeadParams hp, int T, int B, std::vector<float>& dout) {
    if (dev) { arena.reset(); const Win<float> wd = out(dout); actor_head_train_bwd_launch(0, in(keep), hp, T, B, wd.d); finish_launch(); back(wd, dout); return; }
    const float a1 = mut == M_ALPHA_SWAP ? 1 - hp.alpha : hp.alpha, a2 = mut == M_ALPHA_SWAP ? hp.alpha : 1 - hp.alpha;
    for (int b = 0; b < B; ++b) for (int j = 0; j < KBJ_NU; ++j) {
      float gc = 0;
      for (int t = T - 1; t >= 0; --t) {
        if (mut == M_CHUNK && t != T - 1 && (T - 1 - t) % 10 == 0) gc = 0;
        const size_t r = (size_t)t * B + b; const float kp = mut == M_KEEP_BWD ? 1.0f : keep[mut == M_KEEP_NEIGH ? (size_t)std::max(t - 1, 0) * B + b : r];
        const float gy = dout[r * 40 + j] + kp * gc; dout[r * 40 + j] = a1 * gy; gc = a2 * gy;
      }
    }
  }
  // -- group C
  // one block's pair / value as the kernel forms it: per-thread chains, then the LDS tree
  static double block_tree(std::vector<double>& s) { for (int o = 128; o > 0; o >>= 1) for (int t = 0; t < o; ++t) s[t] += s[t + o]; return s[0]; }
  void adv_stats(const std::vector<float>& adv, int R, std::vector<double>& stats, std::vector<double>& part) {
    if (dev) { arena.reset(); const Win<double> ws = out(stats), wp = out(part); adv_stats_launch(0, in(adv), R, ws.d, wp.d); finish_launch(); back(ws, stats); back(wp, part); return; }
    for (int b = 0; b < ADV_STATS_BLOCKS; ++b) {
      std::vector<double> s1(256, 0.0), s2(256, 0.0);
      for (int t = 0; t < 256; ++t) for (int i = b * 256 + t; i < R; i += 256 * ADV_STATS_BLOCKS) { const double v = adv[i]; s1[t] += v; s2[t] += v * v; }
      const double a = block_tree(s1), c = block_tree(s2);
      if (!part.empty()) { part[2 * b] = a; part[2 * b + 1] = c; } else { stats[0] += a; stats[1] += c; }
    }
  }
  void sumsq(const std::vector<float>& g, float scale, std::vector<double>& o, std::vector<double>& part) {
    if (dev) { arena.reset(); const Win<double> wo = out(o), wp = out(part); sumsq_launch(0, in(g), g.size(), scale, wo.d, wp.d); finish_launch(); back(wo, o); back(wp, part); return; }
    for (int b = 0; b < SUMSQ_BLOCKS; ++b) {
      std::vector<double> s(256, 0.0);
      for (int t = 0; t < 256; ++t) for (size_t i = (size_t)b * 256 + t; i < g.size(); i += (size_t)SUMSQ_BLOCKS * 256) { const double v = (double)g[i] * (mut == M_SS_SCALE ? 1.0f : scale); s[t] += v * v; }
      const double a = block_tree(s);
      if (!part.empty()) part[b] = a; else o[0] += a;
    }
  }
  void reduce_double(const std::vector<double>& part, int nblocks, int w, std::vector<double>& o) {
    if (dev) { arena.reset(); const Win<double> wo = out(o); reduce_double_launch(0, in(part), nblocks, w, wo.d); finish_launch(); back(wo, o); return; }
    for (int j = 0; j < w; ++j) o[j] = o[j] + chain(part.data() + j, (size_t)nblocks, (size_t)w);
  }
  void reduce_rows(const std::vector<float>& part, int nparts, int n, std::vector<float>& o) {
    if (dev) { arena.reset(); const Win<float> wo = out(o); reduce_rows_launch(0, in(part), nparts, n, wo.d); finish_launch(); back(wo, o); return; }
    for (int j = 0; j < n; ++j) o[j] = o[j] + chain(part.data() + j, (size_t)nparts, (size_t)n);
  }
  struct LossIO { std::vector<float> logp, value, ent, logp_old, value_old, adv, target; std::vector<double> stats; };
  // the value half of one sample, shared by ppo_loss and critic_head
  void value_half(float v, float vo, float tg, const PpoParams& pp, float inv, float& dval, float& m1) const {
    const float dv = v - vo, dvc = fminf(fmaxf(dv, -pp.vclip), pp.vclip), vcl = vo + dvc;
    const float e1 = (v - tg) * (v - tg), e2 = (vcl - tg) * (vcl - tg);
    const float gv = e1 >= e2 ? (v - tg) : ((fabsf(dv) < pp.vclip || mut == M_VZERO) ? (vcl - tg) : 0.0f);
    dval = (mut == M_VCOEF ? 1.0f : pp.vcoef) * inv * gv; m1 = 0.5f * fmaxf(e1, e2);
  }
  void ppo_loss(const LossIO& x, PpoParams pp, int R, std::vector<float>& dlogp, std::vector<float>& dvalue, std::vector<double>& macc, int part) {
    if (dev) {
      arena.reset(); const Win<float> wl = out(dlogp), wv = out(dvalue); const Win<double> wm = out(macc);
      ppo_loss_launch(0, in(x.logp), in(x.value), in(x.ent), in(x.logp_old), in(x.value_old), in(x.adv), in(x.target), in(x.stats), pp, R, wl.d, wv.d, wm.d, part);
      finish_launch(); back(wl, dlogp); back(wv, dvalue); back(wm, macc); return;
    }
    if (mut == M_PART) part = 3;
    const float inv = 1.0f / (mut == M_INV ? R - 1 : R);
    double m[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < R; ++r) {
      if (part & 1) {
        const double cnt = (x.stats[11] > 0 && mut != M_STATS11) ? x.stats[11] : (double)R;
        const double mean_d = x.stats[0] / cnt, var_d = std::fmax(x.stats[1] / cnt - mean_d * mean_d, 0.0);
        float a;
        if (mean_d * mean_d <= 64.0 * var_d || mut == M_FP32_200) { const float mean = (float)mean_d, var = fmaxf((float)(x.stats[1] / cnt) - mean * mean, 0.0f); a = (x.adv[r] - mean) / (sqrtf(var) + pp.adv_eps); }
        else a = (float)(((double)x.adv[r] - mean_d) / (std::sqrt(var_d) + (double)pp.adv_eps));
        const float d = x.logp[r] - x.logp_old[r], dcl = fminf(fmaxf(d, -pp.lrclip), pp.lrclip), ratio = expf(dcl);
        float rc = fminf(fmaxf(ratio, 1 - pp.clip), 1 + pp.clip);
        if (mut == M_CLIP_D) rc = fabsf(d) > pp.clip ? (d > 0 ? 1 + pp.clip : 1 - pp.clip) : ratio;
        const float s1 = ratio * a, s2 = rc * a; const bool unclipped = s1 <= s2;
        dlogp[r] = (unclipped && fabsf(d) < pp.lrclip) ? -inv * a * ratio : 0.0f;
        m[0] += (double)-(unclipped ? s1 : s2); m[2] += (double)x.ent[r]; m[3] += (mut == M_CLIP_D ? fabsf(d) : fabsf(ratio - 1)) > pp.clip ? 1.0 : 0.0; m[4] += (double)-d;
      }
      if (part & 2) { float dval, m1; value_half(x.value[r], x.value_old[r], x.target[r], pp, inv, dval, m1); dvalue[r] = dval; m[1] += (double)m1; }
    }
    for (int k = 0; k < 5; ++k) if (k == 1 ? (part & 2) : (part & 1)) macc[k] += m[k];
  }
  void critic_head(int H, const std::vector<float>& h, const std::vector<float>& w, const std::vector<float>& b, const std::vector<float>& vo, const std::vector<float>& tg, PpoParams pp, int R,
                   std::vector<float>& value, std::vector<float>& dvalue, std::vector<float>& dout, std::vector<float>& dh, std::vector<double>& macc) {
    if (dev) {
      arena.reset(); const Win<float> wv = out(value), wd = out(dvalue), wo = out(dout), wh = out(dh); const Win<double> wm = out(macc);
      if (!critic_head_launch(0, H, in(h), in(w), in(b), in(vo), in(tg), pp, R, wv.d, wd.d, wo.d, wh.d, wm.d)) { printf("critic_head_launch: no kernel for H=%d\n", H); exit(1); }
      finish_launch(); back(wv, value); back(wd, dvalue); back(wo, dout); back(wh, dh); back(wm, macc); return;
    }
    const float inv = 1.0f / (mut == M_INV ? R - 1 : R); double m1s = 0;
    for (int r = 0; r < R; ++r) {
      float s = 0; for (int k = 0; k < H; ++k) s += h[(size_t)r * H + k] * w[k];
      const float v = s + (mut == M_CH_BIAS ? 0.0f : b[0]); float dval, m1; value_half(v, vo[r], tg[r], pp, inv, dval, m1);
      value[r] = v; dvalue[r] = dval; dout[(size_t)r * 40 + (mut == M_CH_DOUT ? 1 : 0)] = dval; m1s += (double)m1;
    }
    for (int r = 0; r < R; ++r) for (int k = 0; k < H; ++k) dh[(size_t)r * H + k] = dvalue[mut == M_CH_DH ? (r + 1) % R : r] * w[k];
    macc[1] += m1s;
  }
  void critic_value(const std::vector<float>& o, int ld, int N, std::vector<float>& value) {
    if (dev) { arena.reset(); const Win<float> wv = out(value); critic_value_launch(0, in(o), ld, N, wv.d); finish_launch(); back(wv, value); return; }
    for (int n = 0; n < N; ++n) value[n] = o[(size_t)n * ld];
  }
  void mirror_loss(const std::vector<float>& y, const std::vector<float>& ym, const std::vector<float>& v, const std::vector<float>& vm, float sa, float sc, int R, std::vector<float>& dy,
                   std::vector<float>& dym, std::vector<float>& dvalue, std::vector<float>& dvalue_m, std::vector<double>& macc, int part) {
    if (dev) {
      arena.reset(); const Win<float> w1 = out(dy), w2 = out(dym), w3 = out(dvalue), w4 = out(dvalue_m); const Win<double> wm = out(macc);
      mirror_loss_launch(0, in(y), in(ym), in(v), in(vm), sa, sc, R, w1.d, w2.d, w3.d, w4.d, wm.d, part); finish_launch();
      back(w1, dy); back(w2, dym); back(w3, dvalue); back(w4, dvalue_m); back(wm, macc); return;
    }
    if (mut == M_PART) part = 3;
    for (int r = 0; r < R; ++r) {
      const float ca = sa / (20.0f * R); float la = 0;
      if (part & 1) {
        for (int i = 0; i < KBJ_NU; ++i) {
          const int s = mut == M_MIR_MAP ? i : (i < 5 ? i + 5 : (i < 10 ? i - 5 : i));
          const float e = mut == M_MIR_SIGN ? y[(size_t)r * KBJ_NU + i] - ym[(size_t)r * KBJ_NU + s] : y[(size_t)r * KBJ_NU + i] + ym[(size_t)r * KBJ_NU + s];
          la += e * e; dy[(size_t)r * KBJ_NU + i] = 2 * ca * e; dym[(size_t)r * KBJ_NU + s] = 2 * ca * e;
        }
        macc[5] += (double)(sa * la / 20.0f);
      }
      if (part & 2) { const float ev = v[r] - vm[r], gv = 2 * sc / R * ev; dvalue[r] += gv; dvalue_m[r] = -gv; macc[6] += (double)(sc * ev * ev); }
    }
  }
  void metrics(const std::vector<double>& macc, const std::vector<double>& stats, PpoParams pp, int R, std::vector<float>& m) {
    if (dev) { arena.reset(); const Win<float> wm = out(m); ppo_metrics_launch(0, in(macc), in(stats), pp, R, wm.d); finish_launch(); back(wm, m); return; }
    const double pol = macc[0] / R, vl = macc[1] / R, en = macc[2] / R, ma = macc[5] / R, mc = macc[6] / R, cnt = stats[11] > 0 ? stats[11] : (double)R;
    const double mean = stats[0] / cnt, var = stats[1] / cnt - mean * mean;
    m[0] = (float)(pol + pp.vcoef * vl - pp.ecoef * en + ma + mc); m[8] = (float)ma; m[9] = (float)mc; m[1] = (float)pol; m[2] = (float)vl; m[3] = (float)en;
    m[4] = (float)(macc[3] / R); m[5] = (float)(macc[4] / R); m[6] = (float)mean; m[7] = (float)std::sqrt(var > 0 ? var : 0);
  }
  // -- group D
  void matvec(const std::vector<float>& W, const std::vector<float>& x, const std::vector<float>& add, int M, int K, std::vector<float>& y) {
    if (dev) { arena.reset(); const Win<float> wy = out(y); matvec_launch(0, in(W), in(x), in(add), M, K, wy.d); finish_launch(); back(wy, y); return; }
    for (int m = 0; m < M; ++m) {
      float s[64]; for (int l = 0; l < 64; ++l) { s[l] = 0; for (int k = l; k < K; k += 64) s[l] += W[(size_t)m * K + k] * x[k]; }
      for (int o = 32; o > 0; o >>= 1) for (int l = 0; l < o; ++l) s[l] += s[l + o];
      y[m] = s[0] + (add.empty() ? 0.0f : add[m]);
    }
  }
  void matvec_t(const std::vector<float>& W, const std::vector<float>& x, int K, int N, std::vector<float>& y, std::vector<float>& part) {
    if (dev) { arena.reset(); const Win<float> wy = out(y), wp = out(part); matvec_t_acc_launch(0, in(W), in(x), K, N, wy.d, wp.d); finish_launch(); back(wy, y); back(wp, part); return; }
    for (int by = 0; by < MATVEC_T_SLICES; ++by) for (int n = 0; n < N; ++n) {
      float p[4]; for (int ph = 0; ph < 4; ++ph) { p[ph] = 0; for (int k = ph + 4 * by; k < K; k += 4 * MATVEC_T_SLICES) p[ph] += W[(size_t)k * N + n] * x[k]; }
      const float v = p[0] + p[1] + p[2] + p[3];
      if (!part.empty()) part[(size_t)by * N + n] = v; else y[n] += v;
    }
  }
  void outer_acc(std::vector<float>& C, const std::vector<float>& u, const std::vector<float>& v, int M, int N) {
    if (dev) { arena.reset(); const Win<float> wc = out(C); outer_acc_launch(0, wc.d, in(u), in(v), M, N); finish_launch(); back(wc, C); return; }
    for (int m = 0; m < M; ++m) for (int n = 0; n < N; ++n) C[(size_t)m * N + n] += u[m] * v[n];
  }
  void colsum(const std::vector<float>& X, int M, int N, int ld, std::vector<float>& o, std::vector<float>& part) {
    if (dev) { arena.reset(); const Win<float> wo = out(o), wp = out(part); colsum_launch(0, in(X), M, N, ld, wo.d, wp.d); finish_launch(); back(wo, o); back(wp, part); return; }
    const int l = mut == M_CS_LD ? N : ld;
    for (int by = 0; by < DETP_ROWS; ++by) for (int c = 0; c < N; ++c) {
      float p[4]; for (int ph = 0; ph < 4; ++ph) { p[ph] = 0; if (!(mut == M_CS_PHASE && ph == 3)) for (int m = ph + 4 * by; m < M; m += 4 * DETP_ROWS) p[ph] += X[(size_t)m * l + c]; }
      const float v = p[0] + p[1] + p[2] + p[3];
      if (!part.empty()) part[(size_t)by * N + c] = v; else o[c] += v;
    }
  }
};

// ---- driver --------------------------------------------------------------------------------------------------------------------------------
static std::map<std::string, std::map<std::string, double>> worst_frac;   // kernel -> category -> worst fraction of the bound on the device
static std::map<std::string, int> case_count;
static std::string fractions(const Chk& k) { std::string s; char b[64]; for (auto& kv : k.worst) { snprintf(b, sizeof b, " %s %.3f", kv.first.c_str(), kv.second); s += b; } return s; }
// one case: run(ops) executes the case's launches through `ops`, check() judges what they left
static void run_case(const char* kernel, const char* what, const Muts& muts, const std::function<void(Ops&)>& run, const std::function<Chk()>& check, const std::string& live = "", bool live_ok = true) {
  cur_kernel = kernel; cur_what = what; ++case_count[kernel];
  Ops ops;
  if (!tally.plan_mode) {
    ops.dev = true; run(ops);
    Chk k = check(); if (!ops.guards) k.fail("guards", "stray store (guard changed)");
    const bool ok = live_ok && k.mx <= 1.0;
    for (auto& kv : k.worst) { double& w = worst_frac[kernel][kv.first]; w = std::max(w, kv.second); }
    printf("case %-12s %-60s : %s%s%s\n", kernel, what, ok ? "ok" : "FAIL ", ok ? fractions(k).c_str() : (k.mx > 1.0 ? k.why : "inputs not live"), ok ? live.c_str() : "");
    tally.count(ok); return;
  }
  std::string line = live; char b[260]; bool ok = live_ok;
  if (!live_ok) line += " FAIL inputs not live;";
  run(ops);
  const Chk k0 = check();
  if (k0.mx <= 1.0) line += " model ok"; else { ok = false; snprintf(b, sizeof b, " model FAIL (%s);", k0.why); line += b; }
  for (auto& m : muts) {
    if (!m.second) { line += std::string(" ") + MUTN[m.first] + "=n/a"; continue; }
    Ops mo; mo.mut = m.first; run(mo);
    const double r = check().mx;
    if (r > 100.0) line += std::string(" ") + MUTN[m.first] + "=rejected";
    else { ok = false; snprintf(b, sizeof b, " %s=FAIL (passes within %.3g x bound)", MUTN[m.first], r); line += b; }
  }
  printf("case %-12s %-60s : %s%s\n", kernel, what, ok ? "planned" : "FAIL", line.c_str());
  tally.count(ok);
}
static uint32_t next_id = 1;

// a hashed subset of B rows out of N that always holds N - 1 and (B >= 2) 0
static std::vector<int> make_idx(int N, int B, uint32_t tag, bool repeat = false) {
  std::vector<std::pair<uint32_t, int>> o(N); for (int n = 0; n < N; ++n) o[n] = {hash3(tag, n, 7), n};
  std::sort(o.begin(), o.end());
  std::vector<int> idx(B); for (int b = 0; b < B; ++b) idx[b] = o[b].second;
  if (std::find(idx.begin(), idx.end(), N - 1) == idx.end()) idx[0] = N - 1;
  if (B >= 2 && std::find(idx.begin(), idx.end(), 0) == idx.end()) idx[idx[0] == N - 1 ? 1 : 0] = 0;
  if (B >= 2 && idx[0] == 0 && N > 1) std::swap(idx[0], idx[1]);   // idx[0] != 0: the identity never matches
  if (repeat && B >= 3) idx[2] = idx[0];
  return idx;
}
static bool idx_differs(const std::vector<int>& idx) { for (size_t b = 0; b < idx.size(); ++b) if (idx[b] != (int)b) return true; return false; }

// ---- group A -------------------------------------------------------------------------------------------------------------------------------
static void gather_rows_case(int T, int N, int B, int wdt, int lds, int ldd, bool scalar, bool repeat) {
  const uint32_t tag = 0x41000000u + 16u * next_id++;
  char what[120]; snprintf(what, sizeof what, "T=%d N=%d B=%d w=%d lds=%d ldd=%d form=%s%s", T, N, B, wdt, lds, ldd, scalar ? "rows" : "rows4", repeat ? " repeat" : "");
  std::vector<float> src; fill(src, (size_t)T * N * lds, tag, 1.0f);
  const std::vector<int> idx = make_idx(N, B, tag + 1, repeat);
  std::vector<float> dst;
  auto run = [&](Ops& o) { dst = pat((size_t)T * B * ldd); o.gather_rows(src, idx, T, N, B, wdt, lds, ldd, dst, scalar); };
  auto check = [&]() { Chk k; for (int t = 0; t < T; ++t) for (int b = 0; b < B; ++b) for (int c = 0; c < ldd; ++c)
      k.exact(c < wdt ? "copy" : "padding", dst[((size_t)t * B + b) * ldd + c], c < wdt ? src[((size_t)t * N + idx[b]) * lds + c] : PATTERN, t * B + b, c); return k; };
  run_case(scalar ? "gather_rows" : "gather_rows4", what, Muts{{M_IDX, idx_differs(idx)}, {M_TSTRIDE, T > 1 && B != N}}, run, check);
}
static void gather_small_case(int T, int N, int B, int c0, int c1, bool nulls) {
  const uint32_t tag = 0x42000000u + 16u * next_id++;
  char what[120]; snprintf(what, sizeof what, "T=%d N=%d B=%d cols=[%d,%d) old=%s", T, N, B, c0, c1, nulls ? "null" : "given");
  SmallIO s; const size_t TN = (size_t)T * N, R = (size_t)T * B;
  fill(s.action, TN * KBJ_NU, tag, 1.0f); fill(s.aux, TN * KBJ_AUX_SIZE, tag + 1, 1.0f);
  if (!nulls) { fill(s.logp, TN, tag + 2, 1.0f); fill(s.value, TN, tag + 3, 1.0f); fill(s.adv, TN, tag + 4, 1.0f); fill(s.target, TN, tag + 5, 1.0f); }
  static const float DV[4] = {0.0f, 1.0f, -1.0f, -0.0f};
  for (size_t r = 0; r < TN; ++r) s.aux[r * KBJ_AUX_SIZE + KBJ_AUX_DONE] = DV[r < 4 ? r : hash3(tag + 6, (uint32_t)r, 0) % 4u];
  const std::vector<int> idx = make_idx(N, B, tag + 7);
  auto run = [&](Ops& o) { s.action_o = pat(R * KBJ_NU); s.logp_o = pat(R); s.value_o = pat(R); s.adv_o = pat(R); s.target_o = pat(R); s.keep_o = pat(R); o.gather_small(s, idx, T, N, B, c0, c1); };
  auto check = [&]() {
    Chk k; auto on = [&](int c) { return c >= c0 && c < c1; };
    for (int t = 0; t < T; ++t) for (int b = 0; b < B; ++b) {
      const size_t r = (size_t)t * B + b, q = (size_t)t * N + idx[b];
      for (int c = 0; c < KBJ_NU; ++c) k.exact("action", s.action_o[r * KBJ_NU + c], on(c) ? s.action[q * KBJ_NU + c] : PATTERN, r, c);
      k.exact("logp", s.logp_o[r], on(20) && !nulls ? s.logp[q] : PATTERN, r, 20); k.exact("value", s.value_o[r], on(21) && !nulls ? s.value[q] : PATTERN, r, 21);
      k.exact("adv", s.adv_o[r], on(22) && !nulls ? s.adv[q] : PATTERN, r, 22); k.exact("target", s.target_o[r], on(23) && !nulls ? s.target[q] : PATTERN, r, 23);
      k.exact("keep", s.keep_o[r], on(24) ? (s.aux[q * KBJ_AUX_SIZE + KBJ_AUX_DONE] != 0 ? 0.0f : 1.0f) : PATTERN, r, 24);
    }
    return k;
  };
  run_case("gather_small", what, Muts{{M_IDX, idx_differs(idx)}, {M_TSTRIDE, T > 1 && B != N}}, run, check);
}
static void gather_carry_case(int nplanes, int nlpf, int H, int B) {
  const uint32_t tag = 0x43000000u + 64u * next_id++; const int N = 70;
  char what[120]; snprintf(what, sizeof what, "planes=%d lpf=%d H=%d B=%d N=%d", nplanes, nlpf, H, B, N);
  std::vector<std::vector<float>> src(nplanes + nlpf), dst;
  for (int p = 0; p < nplanes + nlpf; ++p) fill(src[p], (size_t)N * (p < nplanes ? H : KBJ_NU), tag + p, 1.0f);
  const std::vector<int> idx = make_idx(N, B, tag + 40);
  auto run = [&](Ops& o) { dst.assign(nplanes + nlpf, {}); for (int p = 0; p < nplanes + nlpf; ++p) dst[p] = pat((size_t)B * (p < nplanes ? H : KBJ_NU)); o.gather_carry(src, dst, nplanes, nlpf, idx, B, H); };
  auto check = [&]() { Chk k; for (int p = 0; p < nplanes + nlpf; ++p) { const int w = p < nplanes ? H : KBJ_NU; for (int b = 0; b < B; ++b) for (int c = 0; c < w; ++c) k.exact("copy", dst[p][(size_t)b * w + c], src[p][(size_t)idx[b] * w + c], p * 1000 + b, c); } return k; };
  run_case("gather_carry", what, Muts{{M_IDX, true}}, run, check);
}
static void mirror_rows_case(bool critic, int rows) {
  const uint32_t tag = 0x44000000u + 16u * next_id++;
  kbj_model m{};
  for (int j = 0; j < KBJ_NU; ++j) { m.joint_bias[j] = 0.6f * hv(0x4400FFF0u, j); m.joint_lo[j] = m.joint_bias[j] - 0.5f - 1.5f * hu(0x4400FFF1u, j); m.joint_hi[j] = m.joint_bias[j] + 0.5f + 1.5f * hu(0x4400FFF2u, j); }
  std::vector<MirrorEntry> ta, tc; build_mirror_tables(m, ta, tc);
  const std::vector<MirrorEntry>& tab = critic ? tc : ta; const int ld = (int)tab.size();
  char what[120]; snprintf(what, sizeof what, "table=%s ld=%d rows=%d", critic ? "critic" : "actor", ld, rows);
  std::vector<float> x, y; fill(x, (size_t)rows * ld, tag, 1.0f);
  auto run = [&](Ops& o) { y = pat((size_t)rows * ld); o.mirror_rows(x, y, rows, ld, tab); };
  auto check = [&]() {
    Chk k;
    for (int r = 0; r < rows; ++r) for (int c = 0; c < ld; ++c) {
      const MirrorEntry e = tab[c]; const double xi = x[(size_t)r * ld + e.src], ref = (double)e.mul * xi + e.add; const float got = y[(size_t)r * ld + c];
      if (std::fabs(e.mul) == 1.0f && e.add == 0.0f) k.exact("signed_copy", got, e.mul * x[(size_t)r * ld + e.src], r, c);
      else k.upd("affine", std::fabs(got - ref), U * std::fabs(e.mul * xi) + U * std::fabs(ref), r, c);
    }
    return k;
  };
  run_case("mirror_rows", what, Muts{}, run, check);
}
static void repitch_rows_case(int rows, int cols, int ld) {
  const uint32_t tag = 0x45000000u + 16u * next_id++; char what[120]; snprintf(what, sizeof what, "rows=%d cols=%d ld=%d", rows, cols, ld);
  std::vector<float> src, dst; fill(src, (size_t)rows * cols, tag, 1.0f);
  auto run = [&](Ops& o) { dst = pat((size_t)rows * ld); o.repitch_rows(src, rows, cols, ld, dst); };
  auto check = [&]() { Chk k; for (int r = 0; r < rows; ++r) for (int c = 0; c < ld; ++c) k.exact("copy", dst[(size_t)r * ld + c], c < cols ? src[(size_t)r * cols + c] : 0.0f, r, c); return k; };
  run_case("repitch_rows", what, Muts{}, run, check);
}
static void repitch_pad_case(int rows, int ws, int wd) {
  const uint32_t tag = 0x46000000u + 16u * next_id++; char what[120]; snprintf(what, sizeof what, "rows=%d ws=%d wd=%d", rows, ws, wd);
  std::vector<float> src, dst; fill(src, (size_t)rows * ws, tag, 1.0f);
  auto run = [&](Ops& o) { dst = pat((size_t)rows * wd); o.repitch_pad(src, dst, rows, ws, wd); };
  auto check = [&]() { Chk k; for (int r = 0; r < rows; ++r) for (int c = 0; c < wd; ++c) k.exact("copy", dst[(size_t)r * wd + c], c < ws ? src[(size_t)r * ws + c] : 0.0f, r, c); return k; };
  run_case("repitch_pad", what, Muts{}, run, check);
}

// ---- group B -------------------------------------------------------------------------------------------------------------------------------
enum KeepPat { K_NONE = 0, K_ALL, K_HASH, K_SINGLE };
static const char* KEEPN[4] = {"none", "all", "hashed", "single"};
static HeadParams default_hp(int ld) { return HeadParams{0.01f, 1.0f, 0.5f, 0.02f / (0.02f + 1.0f / (6.2831853f * 10.0f)), ld}; }
struct HeadB {
  int T = 0, B = 0, R = 0, ld = 68, kp = K_HASH; HeadParams hp{}; bool extra = false, mirror = false, chained = false; float dent = 0;
  std::vector<float> out, obs, jb, keep, lpf0, act, dlogp, dy;              // inputs
  std::vector<float> y0, sd, y, lp, en, dpre, dout;                          // stage outputs
  std::vector<float> y_steps, dout_steps;                                    // links: one-step launches
  std::vector<std::pair<int, std::vector<float>>> prefixes;                  // (t0, dout of a launch over [0, t0))
  std::vector<int> rows; std::vector<std::vector<float>> row_y, row_dout;    // rows relaunched alone
  int redraws = 0; long viol = 0; double clamp_share = 0;
};
static double pre_of(const HeadParams& hp, double raw, double& e) {   // (softplus + min_std) var_scale and its fp32 error bound
  const double sp = raw > 30.0 ? raw : std::log1p(std::exp(raw)), e_sp = 6 * U / (1.0 + std::exp(-raw)) + 4 * U * sp;
  e = hp.var_scale * e_sp + 2 * U * (sp + hp.min_std) * hp.var_scale; return (sp + hp.min_std) * (double)hp.var_scale;
}
static void make_headb(HeadB& p, uint32_t id) {
  const uint32_t tag = 0x48000000u + 16u * id; const int T = p.T, B = p.B, R = T * B; p.R = R; p.hp.ld_obs = p.ld;
  fill(p.out, (size_t)R * 40, tag, 1.0f); fill(p.obs, (size_t)R * p.ld, tag + 1, 1.0f); fill(p.jb, KBJ_NU, tag + 2, 0.5f); fill(p.lpf0, (size_t)B * KBJ_NU, tag + 3, 1.0f);
  fill(p.act, (size_t)R * KBJ_NU, tag + 4, 1.5f); fill(p.dlogp, R, tag + 5, 1.0f / R); if (p.extra || p.mirror) fill(p.dy, (size_t)R * KBJ_NU, tag + 6, 1.0f / R);
  if (p.mirror) std::fill(p.dlogp.begin(), p.dlogp.end(), 0.0f);
  for (int r = 0; r < R; ++r) for (int c = KBJ_NOBS_ACTOR; c < p.ld; ++c) p.obs[(size_t)r * p.ld + c] = QNAN;
  const float centre = (float)softplus_inv((double)p.hp.max_std / p.hp.var_scale - p.hp.min_std); long on = 0;
  for (int r = 0; r < R; ++r) for (int j = 0; j < KBJ_NU; ++j) {
    for (uint32_t salt = 0;; ++salt) {
      const float raw = centre + 2.0f * hv(tag + 7, (size_t)r * KBJ_NU + j, salt); double e; const double pre = pre_of(p.hp, raw, e);
      if (std::fabs(pre - p.hp.max_std) > MARGIN * e) { p.out[(size_t)r * 40 + KBJ_NU + j] = raw; on += pre >= p.hp.max_std; break; }
      ++p.redraws;
    }
  }
  for (int r = 0; r < R; ++r) for (int j = 0; j < KBJ_NU; ++j) { double e; const double pre = pre_of(p.hp, p.out[(size_t)r * 40 + KBJ_NU + j], e); p.viol += !(std::fabs(pre - p.hp.max_std) > MARGIN * e); }
  p.clamp_share = (double)on / ((double)R * KBJ_NU);
  p.keep.assign(R, 1.0f);
  for (int t = 0; t < T; ++t) for (int b = 0; b < B; ++b) {
    float& k = p.keep[(size_t)t * B + b];
    if (p.kp == K_ALL) k = 0.0f; else if (p.kp == K_HASH) k = hash3(tag + 8, t, b) % 5u == 0 ? 0.0f : 1.0f; else if (p.kp == K_SINGLE) k = (t == 9 || t == 10) ? 0.0f : 1.0f;
  }
  if (p.kp == K_HASH && T > 1) { p.keep[0] = 0.0f; p.keep[B] = 1.0f; }   // row 0: a reset at t = 0 and none at t = 1 (what the keep mutants are exercised by)
  p.rows.clear(); if (B > 1) { p.rows = {0, B / 2, B - 1}; }
}
static std::vector<float> rows_of(const std::vector<float>& v, int T, int B, int w, int b) {   // [T][B][w] -> row b as [T][1][w]
  std::vector<float> o((size_t)T * w); for (int t = 0; t < T; ++t) std::copy(v.begin() + ((size_t)t * B + b) * w, v.begin() + ((size_t)t * B + b + 1) * w, o.begin() + (size_t)t * w); return o;
}
static void run_headb(HeadB& p, Ops& o) {
  const int T = p.T, B = p.B, R = p.R; const size_t RJ = (size_t)R * KBJ_NU;
  p.y0 = pat(RJ); p.sd = pat(RJ); o.head_pre(p.out, p.obs, p.jb, p.hp, R, p.y0, p.sd);
  p.y = p.y0; o.train_fwd(p.keep, p.lpf0, p.hp, T, B, p.y);
  p.lp = pat(R); p.en = pat(R); o.logp(p.y, p.sd, p.act, R, p.lp, p.en);
  p.dpre = pat((size_t)R * 40); o.bwd_pre(p.out, p.y, p.sd, p.act, p.mirror, p.dlogp, p.dy, p.dent, p.hp, R, p.dpre);
  p.dout = p.dpre; o.train_bwd(p.keep, p.hp, T, B, p.dout);
  // links: one-step launches, chained by the host (forward) / on their own (backward)
  p.y_steps = p.y0; p.dout_steps = p.dpre; std::vector<float> state = p.lpf0;
  for (int t = 0; t < T; ++t) {
    std::vector<float> ys(p.y0.begin() + (size_t)t * B * KBJ_NU, p.y0.begin() + (size_t)(t + 1) * B * KBJ_NU), ks(p.keep.begin() + (size_t)t * B, p.keep.begin() + (size_t)(t + 1) * B);
    o.train_fwd(ks, state, p.hp, 1, B, ys); std::copy(ys.begin(), ys.end(), p.y_steps.begin() + (size_t)t * B * KBJ_NU);
    for (int b = 0; b < B; ++b) for (int j = 0; j < KBJ_NU; ++j) state[(size_t)b * KBJ_NU + j] = ks[b] != 0.0f ? ys[(size_t)b * KBJ_NU + j] * ks[b] : 0.0f;
    std::vector<float> ds(p.dpre.begin() + (size_t)t * B * 40, p.dpre.begin() + (size_t)(t + 1) * B * 40);
    o.train_bwd(ks, p.hp, 1, B, ds); std::copy(ds.begin(), ds.end(), p.dout_steps.begin() + (size_t)t * B * 40);
  }
  p.prefixes.clear();
  for (int t0 : {9, 10, 11, T - 1}) if (t0 >= 1 && t0 < T && (p.prefixes.empty() || p.prefixes.back().first != t0)) {
    std::vector<float> d(p.dpre.begin(), p.dpre.begin() + (size_t)t0 * B * 40), ks(p.keep.begin(), p.keep.begin() + (size_t)t0 * B);
    o.train_bwd(ks, p.hp, t0, B, d); p.prefixes.push_back({t0, d});
  }
  p.row_y.clear(); p.row_dout.clear();
  for (int b : p.rows) {
    std::vector<float> y = rows_of(p.y0, T, B, KBJ_NU, b), ks = rows_of(p.keep, T, B, 1, b), l0(p.lpf0.begin() + (size_t)b * KBJ_NU, p.lpf0.begin() + (size_t)(b + 1) * KBJ_NU), d = rows_of(p.dpre, T, B, 40, b);
    o.train_fwd(ks, l0, p.hp, T, 1, y); o.train_bwd(ks, p.hp, T, 1, d); p.row_y.push_back(y); p.row_dout.push_back(d);
  }
}
// chain = false: every stage against the reference formed from ITS stored inputs; true: the whole chain from the raw inputs, bounds propagated
static void check_headb_mode(const HeadB& p, bool chain, Chk& k) {
  const int T = p.T, B = p.B, R = p.R; const HeadParams& hp = p.hp; const double al = hp.alpha;
  const char* C_Y0 = chain ? "chain_y0" : "pre_y"; const char* C_SD = chain ? "chain_sd" : "pre_sd"; const char* C_Y = chain ? "chain_y" : "fwd"; const char* C_LP = chain ? "chain_logp" : "logp";
  const char* C_EN = chain ? "chain_ent" : "ent"; const char* C_DP = chain ? "chain_bwd_pre" : "bwd_pre"; const char* C_D = chain ? "chain_dout" : "bwd";
  const size_t RJ = (size_t)R * KBJ_NU;
  std::vector<double> mv(RJ), me(RJ, 0.0), sv(RJ), se(RJ, 0.0), yv(RJ), ye(RJ, 0.0); std::vector<char> clamp(RJ);
  for (int r = 0; r < R; ++r) for (int j = 0; j < KBJ_NU; ++j) {
    const size_t i = (size_t)r * KBJ_NU + j;
    const double o = p.out[(size_t)r * 40 + j], cmd = j >= 10 ? p.obs[(size_t)r * p.ld + KBJ_OBS_CMD + 6 + (j - 10)] : 0.0, m = o + p.jb[j] + cmd, e_m = 2 * U * (std::fabs(o) + std::fabs(p.jb[j]) + std::fabs(cmd));
    double e_pre; const double pre = pre_of(hp, p.out[(size_t)r * 40 + KBJ_NU + j], e_pre); clamp[i] = pre >= hp.max_std;
    k.upd(C_Y0, std::fabs(p.y0[i] - m), e_m, r, j);
    if (clamp[i]) k.exact("clamp", p.sd[i], hp.max_std, r, j); else k.upd(C_SD, std::fabs(p.sd[i] - pre), e_pre, r, j);
    if (chain) { mv[i] = m; me[i] = e_m; sv[i] = clamp[i] ? (double)hp.max_std : pre; se[i] = clamp[i] ? 0.0 : e_pre; } else { mv[i] = p.y0[i]; sv[i] = p.sd[i]; }
  }
  for (int b = 0; b < B; ++b) for (int j = 0; j < KBJ_NU; ++j) {
    double s = p.lpf0[(size_t)b * KBJ_NU + j], e_s = 0;
    for (int t = 0; t < T; ++t) {
      const size_t i = ((size_t)t * B + b) * KBJ_NU + j; const double kp = p.keep[(size_t)t * B + b];
      const double y = s + al * (mv[i] - s), e = (1 - al) * e_s + al * me[i] + al * U * std::fabs(mv[i] - s) + U * std::fabs(al * (mv[i] - s)) + U * std::fabs(y);
      k.upd(C_Y, std::fabs(p.y[i] - y), SECOND_ORDER * e, t * B + b, j);
      if (chain) { yv[i] = y; ye[i] = e; s = y * kp; e_s = e * kp; } else { yv[i] = p.y[i]; s = (double)p.y[i] * kp; e_s = 0; }
    }
  }
  std::vector<double> gv((size_t)R * KBJ_NU), ge((size_t)R * KBJ_NU);
  for (int r = 0; r < R; ++r) {
    double lp = 0, lp_abs = 0, lp_e = 0, en = 0, en_abs = 0, en_e = 0;
    for (int j = 0; j < KBJ_NU; ++j) {
      const size_t i = (size_t)r * KBJ_NU + j; const double s = sv[i], rel = se[i] / (s - se[i]);
      { const double d = (double)p.act[i] - yv[i], z = d / s, e_z = (ye[i] + U * std::fabs(d)) / s + std::fabs(z) * rel + U * std::fabs(z), ls = std::log(s);
        const double t = -0.5 * z * z - ls - HALF_LOG2PI; lp += t; lp_abs += std::fabs(t);
        lp_e += std::fabs(z) * e_z + e_z * e_z + rel + 6 * U * std::fabs(ls) + 4 * U * (0.5 * z * z + std::fabs(ls) + HALF_LOG2PI);
        const double u = 0.5 + HALF_LOG2PI + ls; en += u; en_abs += std::fabs(u); en_e += rel + 6 * U * std::fabs(ls) + 2 * U * (0.5 + HALF_LOG2PI + std::fabs(ls)); }
      // backward, stage 1 (the mirror form passes y as the action: z = 0 exactly)
      const double d = p.mirror ? 0.0 : (double)p.act[i] - yv[i], z = d / s, e_z = p.mirror ? 0.0 : (ye[i] + U * std::fabs(d)) / s + std::fabs(z) * rel + U * std::fabs(z);
      const double gl = p.dlogp[r], dy = p.dy.empty() ? 0.0 : p.dy[i], t1 = gl * z / s, dm = t1 + dy;
      const double e_dm = std::fabs(gl) * (e_z / s + std::fabs(z / s) * rel) + 2 * U * std::fabs(t1) + U * (std::fabs(t1) + std::fabs(dy));
      k.upd(C_DP, std::fabs(p.dpre[(size_t)r * 40 + j] - dm), SECOND_ORDER * e_dm, r, j);
      gv[i] = chain ? dm : (double)p.dpre[(size_t)r * 40 + j]; ge[i] = chain ? e_dm : 0.0;
      const double zz = z * z, e_zz = 2 * std::fabs(z) * e_z + e_z * e_z + U * zz, q = (zz - 1) / s, e_q = (e_zz + U * std::fabs(zz - 1)) / s + std::fabs(q) * rel + U * std::fabs(q);
      const double ds = p.dent / s, gs = gl * q + ds, e_gs = std::fabs(gl) * e_q + U * std::fabs(gl * q) + std::fabs(ds) * (rel + U) + U * std::fabs(gs) + U * (std::fabs(gl * q) + std::fabs(ds));
      const double raw = p.out[(size_t)r * 40 + KBJ_NU + j], sig = 1.0 / (1.0 + std::exp(-raw)), dstd = gs * hp.var_scale * sig;
      if (clamp[i]) k.exact("clamp", p.dpre[(size_t)r * 40 + KBJ_NU + j], 0.0f, r, KBJ_NU + j);
      else k.upd(C_DP, std::fabs(p.dpre[(size_t)r * 40 + KBJ_NU + j] - dstd), SECOND_ORDER * (e_gs * hp.var_scale * sig + std::fabs(gs) * hp.var_scale * C_SIG * U + 2 * U * std::fabs(dstd)), r, KBJ_NU + j);
      if (!chain) k.exact("links", p.dout[(size_t)r * 40 + KBJ_NU + j], p.dpre[(size_t)r * 40 + KBJ_NU + j], r, KBJ_NU + j);   // the scan leaves the std columns alone
    }
    k.upd(C_LP, std::fabs(p.lp[r] - lp), SECOND_ORDER * (lp_e + gamma_n(KBJ_NU) * lp_abs), r, 0);
    k.upd(C_EN, std::fabs(p.en[r] - en), SECOND_ORDER * (en_e + gamma_n(KBJ_NU) * en_abs), r, 1);
  }
  for (int b = 0; b < B; ++b) for (int j = 0; j < KBJ_NU; ++j) {
    double gc = 0, e_gc = 0;
    for (int t = T - 1; t >= 0; --t) {
      const size_t i = ((size_t)t * B + b) * KBJ_NU + j; const double kp = p.keep[(size_t)t * B + b];
      const double gy = gv[i] + kp * gc, e_gy = ge[i] + kp * e_gc + U * std::fabs(gy), o = al * gy, e_o = al * e_gy + U * std::fabs(o);
      k.upd(C_D, std::fabs(p.dout[((size_t)t * B + b) * 40 + j] - o), SECOND_ORDER * e_o, t * B + b, j);
      gc = (1 - al) * gy; e_gc = (1 - al) * e_gy + 2 * U * std::fabs(gc);
    }
  }
}
static Chk check_headb(const HeadB& p) {
  Chk k; const int T = p.T, B = p.B;
  check_headb_mode(p, false, k);
  if (p.chained) check_headb_mode(p, true, k);
  k.same("links", p.y_steps, p.y);   // a T-step launch == T one-step launches (a reset restarts from +0)
  for (int t = 0; t < T; ++t) for (int b = 0; b < B; ++b) if (t == T - 1 || p.keep[(size_t)t * B + b] == 0.0f)
    for (int j = 0; j < KBJ_NU; ++j) k.exact("links", p.dout[((size_t)t * B + b) * 40 + j], p.dout_steps[((size_t)t * B + b) * 40 + j], t * B + b, 100 + j);
  for (auto& pf : p.prefixes) for (int b = 0; b < B; ++b) if (p.keep[(size_t)(pf.first - 1) * B + b] == 0.0f)
    for (int t = 0; t < pf.first; ++t) for (int j = 0; j < KBJ_NU; ++j) k.exact("links", p.dout[((size_t)t * B + b) * 40 + j], pf.second[((size_t)t * B + b) * 40 + j], t * B + b, 200 + j);
  for (size_t s = 0; s < p.rows.size(); ++s) {
    if (p.row_y.size() != p.rows.size()) { k.fail("rows", "single-row relaunch missing"); break; }
    const int b = p.rows[s];
    for (int t = 0; t < T; ++t) for (int j = 0; j < KBJ_NU; ++j) { k.exact("rows", p.row_y[s][(size_t)t * KBJ_NU + j], p.y[((size_t)t * B + b) * KBJ_NU + j], t * B + b, j); k.exact("rows", p.row_dout[s][(size_t)t * 40 + j], p.dout[((size_t)t * B + b) * 40 + j], t * B + b, 100 + j); }
  }
  return k;
}
static void headb_case(int T, int B, int ld, const char* hpn, HeadParams hp, int kp, bool extra, bool dent0, bool mirror, bool chained) {
  HeadB p; p.T = T; p.B = B; p.ld = ld; p.hp = hp; p.kp = kp; p.extra = extra; p.mirror = mirror; p.chained = chained; p.dent = (dent0 || mirror) ? 0.0f : -0.004f / (float)(T * B);
  make_headb(p, next_id++);
  char what[140]; snprintf(what, sizeof what, "T=%d B=%d ld=%d hp=%s keep=%s dy=%d dent=%d form=%s%s", T, B, ld, hpn, KEEPN[kp], extra || mirror, p.dent != 0.0f, mirror ? "mirror" : "policy", chained ? " chained" : "");
  char live[120]; snprintf(live, sizeof live, " clamp %.3f redraws %d margin_violations %ld", p.clamp_share, p.redraws, p.viol);
  const bool zeros = kp != K_NONE, mixed = kp == K_HASH || kp == K_SINGLE;
  const Muts muts{{M_CHUNK, T > 10 && hp.alpha != 1.0f}, {M_KEEP_NEIGH, mixed && T > 1 && hp.alpha != 1.0f}, {M_KEEP_BWD, zeros && T > 1 && hp.alpha != 1.0f}, {M_ALPHA_SWAP, true}, {M_CMD_COL, true}, {M_STD_COL, true},
                  {M_CLAMP, true}, {M_CLAMP_DERIV, !mirror}, {M_LOGP19, true}, {M_ENT_GS, p.dent != 0.0f}};
  run_case("actor_train", what, muts, [&](Ops& o) { run_headb(p, o); }, [&]() { return check_headb(p); }, live, p.clamp_share >= 0.1 && p.clamp_share <= 0.9 && p.viol == 0);
}

// ---- group C: the loss's per-sample reference, shared by the generator (margins, liveness) and the checker ------------------------------------
struct ValRef { double gv, e_gv, m1, e_m1, margin; int outcome; bool zero; };   // outcome 0 inactive, 1 active e1 >= e2, 2 active zero
static ValRef value_ref(const PpoParams& pp, double v, double e_v, double vo, double tg) {
  ValRef o{}; const double dv = v - vo, e_dv = e_v + U * std::fabs(dv), vc = pp.vclip;
  const bool active = std::fabs(dv) >= vc; const double vcl = active ? vo + (dv > 0 ? vc : -vc) : v;
  const double a1 = v - tg, e_a1 = e_v + U * std::fabs(a1), a2 = vcl - tg, e_a2 = (active ? 0.0 : e_dv) + U * std::fabs(vcl) + U * std::fabs(a2);
  o.margin = std::fabs(std::fabs(dv) - vc) / e_dv;
  if (!active) { o.outcome = 0; o.gv = a1; o.e_gv = std::max(e_a1, e_v + e_a2); }
  else {
    const double q = std::fabs(a1) - std::fabs(a2), e_q = e_a1 + e_a2 + U * (std::fabs(a1) + std::fabs(a2));
    o.margin = std::min(o.margin, std::fabs(q) / e_q);
    if (q >= 0) { o.outcome = 1; o.gv = a1; o.e_gv = e_a1; } else { o.outcome = 2; o.gv = 0; o.e_gv = 0; o.zero = true; }
  }
  const double e1 = a1 * a1, e2 = a2 * a2;
  o.m1 = 0.5 * std::max(e1, e2); o.e_m1 = 0.5 * std::max(2 * std::fabs(a1) * e_a1 + e_a1 * e_a1 + U * e1, 2 * std::fabs(a2) * (e_v + e_a2) + (e_v + e_a2) * (e_v + e_a2) + U * e2);
  if (!active) o.e_m1 = 0.5 * (2 * (std::fabs(a1) + e_a1 + e_a2) * (e_a1 + e_a2 + e_v) + U * std::max(e1, e2) * 2);   // e1 and e2 agree to rounding here: either may be the maximum
  return o;
}
struct PolRef { double a, e_a, d, e_d, ratio, e_ratio, dlogp, e_dlogp, surr, e_surr, clipfrac, margin; int outcome; bool zero; };   // outcome 0 in range, 1 clipped to zero, 2 clipped but taken, 3 |d| >= lrclip
static PolRef policy_ref(const PpoParams& pp, int R, const double* stats, double adv, double logp, double logp_old) {
  PolRef o{}; const double cnt = stats[11] > 0 ? stats[11] : (double)R, mean = stats[0] / cnt, var = std::fmax(stats[1] / cnt - mean * mean, 0.0), eps = pp.adv_eps;
  const double num = adv - mean, sd = std::sqrt(var);
  if (mean * mean <= 64.0 * var) {
    const double e_var = 6 * U * (var + mean * mean), e_sd = std::sqrt(var + e_var) - std::sqrt(std::fmax(var - e_var, 0.0)) + U * sd, den = sd + eps, e_den = e_sd + U * den, e_num = U * std::fabs(mean) + U * std::fabs(num);
    o.a = num / den; o.e_a = e_num / (den - e_den) + std::fabs(o.a) * e_den / (den - e_den) + U * std::fabs(o.a);
  } else { o.a = num / (sd + eps); o.e_a = U * std::fabs(o.a) + 16 * UD * (std::fabs(adv) + std::fabs(mean)) / (sd + eps); }
  o.d = logp - logp_old; o.e_d = U * std::fabs(o.d);
  const double lr = pp.lrclip, dcl = std::fmin(std::fmax(o.d, -lr), lr); o.ratio = std::exp(dcl); o.e_ratio = 6 * U * o.ratio + (std::fabs(o.d) < lr ? o.ratio * o.e_d : 0.0);
  const double lo = (double)(1 - pp.clip), hi = (double)(1 + pp.clip);
  o.margin = std::min({std::fabs(o.ratio - lo) / o.e_ratio, std::fabs(o.ratio - hi) / o.e_ratio, std::fabs(std::fabs(o.ratio - 1) - (double)pp.clip) / (o.e_ratio + U * std::fabs(o.ratio - 1)),
                       std::fabs(std::fabs(o.d) - lr) / std::max(o.e_d, 1e-300)});
  if (R > 1) o.margin = std::min(o.margin, std::fabs(o.a) / o.e_a);   // R = 1: the numerator is exactly zero in every form
  const bool above = o.ratio > hi, below = o.ratio < lo, unclipped = !(above && o.a > 0) && !(below && o.a < 0), small = std::fabs(o.d) < lr;
  const double rc = above ? hi : (below ? lo : o.ratio);
  o.surr = unclipped ? o.ratio * o.a : rc * o.a; o.e_surr = o.e_a * o.ratio + std::fabs(o.a) * o.e_ratio + U * std::fabs(o.surr);
  o.clipfrac = std::fabs(o.ratio - 1) > (double)pp.clip ? 1.0 : 0.0;
  const double inv = 1.0 / R;
  if (unclipped && small) { o.dlogp = -inv * o.a * o.ratio; o.e_dlogp = inv * (o.e_a * o.ratio + std::fabs(o.a) * o.e_ratio) + 3 * U * std::fabs(o.dlogp); } else { o.dlogp = 0; o.e_dlogp = 0; o.zero = true; }
  o.outcome = !small ? 3 : (!(above || below) ? 0 : (unclipped ? 2 : 1));
  return o;
}
struct Loss {
  int R = 0, part = 3, ratio = 0; bool foreign = false, chained = false; PpoParams pp{}; Ops::LossIO x; std::vector<double> macc0;
  std::vector<float> dlogp, dvalue, dlogp1, dvalue1, dlogp2, dvalue2; std::vector<double> macc, stats_seen;
  int redraws = 0; long viol = 0; double share[7] = {0, 0, 0, 0, 0, 0, 0};
};
static PpoParams default_pp() { return PpoParams{0.2f, 0.2f, 0.5f, 0.004f, 10.0f, 1e-6f}; }
static void draw_policy(Loss& p, uint32_t tag, int r, uint32_t salt) {
  const PpoParams& pp = p.pp; const double l_hi = std::log1p((double)pp.clip), l_lo = -std::log1p(-(double)pp.clip), lr = pp.lrclip;
  const uint32_t cat = hash3(tag + 1, r, salt) % 20u; const double u = hu(tag + 2, r, salt); double sgn = (hash3(tag + 3, r, salt) & 1u) ? 1.0 : -1.0, mag;
  if (cat < 7) mag = 0.9 * u * l_hi; else if (cat == 7) { mag = l_hi + (0.3 + 0.4 * u) * ((double)pp.clip - l_hi); sgn = 1.0; }
  else if (cat < 16) mag = l_lo + (0.25 + 0.5 * u) * std::min(lr - l_lo, 2 * l_lo); else mag = lr * (1.1 + u);
  p.x.logp_old[r] = -20.0f + 10.0f * hv(tag + 4, r, salt); p.x.logp[r] = (float)((double)p.x.logp_old[r] + sgn * mag);
  p.x.adv[r] = 0.7f * (hv(tag + 5, r, salt) + (float)p.ratio * 0.57735027f);   // uniform(-1, 1) has std 1 / sqrt 3
}
static void draw_value(const PpoParams& pp, uint32_t tag, int r, uint32_t salt, double v, float& vo, float& tg) {
  const double u = hu(tag + 7, r, salt), sgn = (hash3(tag + 8, r, salt) & 1u) ? 1.0 : -1.0;
  if (r == 0) {   // sample 0 always has a gradient (clip active, the unclipped error the larger): what the vcoef / inv mutants are caught by at R = 1
    const double dv0 = pp.vclip * (1.2 + 1.8 * u); vo = (float)(v - dv0); tg = (float)(v - dv0 - (0.25 + 0.5 * hu(tag + 10, r, salt)) * pp.vclip); return;
  }
  const double dv = hash3(tag + 6, r, salt) % 10u < 4u ? 0.9 * hv(tag + 9, r, salt) * pp.vclip : sgn * pp.vclip * (1.2 + 1.8 * u);
  vo = (float)(v - dv); tg = (float)(v + 3.0 * pp.vclip * hv(tag + 10, r, salt));
}
static void own_stats(const Loss& p, double* s) { s[0] = s[1] = 0; for (int r = 0; r < p.R; ++r) { const double v = p.x.adv[r]; s[0] += v; s[1] += v * v; } }
static void make_loss(Loss& p, uint32_t id) {
  const uint32_t tag = 0x50000000u + 32u * id; const int R = p.R;
  for (auto* v : {&p.x.logp, &p.x.value, &p.x.ent, &p.x.logp_old, &p.x.value_old, &p.x.adv, &p.x.target}) v->assign(R, 0.0f);
  fill(p.x.ent, R, tag, 3.0f, 20.0f); fill(p.x.value, R, tag + 11, 2.0f);
  std::vector<uint32_t> sp(R, 0), sv(R, 0);
  for (int r = 0; r < R; ++r) { draw_policy(p, tag, r, 0); draw_value(p.pp, tag, r, 0, p.x.value[r], p.x.value_old[r], p.x.target[r]); }
  p.x.stats.assign(16, 0.0);
  for (int r = 0; r < R; ++r) while (value_ref(p.pp, p.x.value[r], 0, p.x.value_old[r], p.x.target[r]).margin <= MARGIN) { draw_value(p.pp, tag, r, ++sv[r], p.x.value[r], p.x.value_old[r], p.x.target[r]); ++p.redraws; }
  for (int pass = 0; pass < 20; ++pass) {   // a re-drawn advantage moves the mean: until a pass re-draws nothing
    if (p.foreign) { const double m = 0.7 * 0.57735027 * p.ratio + 0.05, s = 0.45; p.x.stats[11] = 4.0 * R; p.x.stats[0] = 4.0 * R * m; p.x.stats[1] = 4.0 * R * (s * s + m * m); } else own_stats(p, p.x.stats.data());
    int n = 0;
    for (int r = 0; r < R; ++r) if (policy_ref(p.pp, R, p.x.stats.data(), p.x.adv[r], p.x.logp[r], p.x.logp_old[r]).margin <= MARGIN) { draw_policy(p, tag, r, ++sp[r]); ++n; }
    p.redraws += n; if (!n) break;
  }
  for (int r = 0; r < R; ++r) {
    const PolRef a = policy_ref(p.pp, R, p.x.stats.data(), p.x.adv[r], p.x.logp[r], p.x.logp_old[r]); const ValRef b = value_ref(p.pp, p.x.value[r], 0, p.x.value_old[r], p.x.target[r]);
    p.viol += !(a.margin > MARGIN) + !(b.margin > MARGIN); p.share[a.outcome] += 1.0 / R; p.share[4 + b.outcome] += 1.0 / R;
  }
  p.macc0.resize(8); for (int i = 0; i < 8; ++i) p.macc0[i] = 1.5 + 0.25 * i;
}
static void run_loss(Loss& p, Ops& o) {
  const int R = p.R; Ops::LossIO x = p.x;
  if (p.chained) { std::vector<double> st(16, 0.0), none; o.adv_stats(p.x.adv, R, st, none); x.stats = st; }
  p.stats_seen = x.stats;
  p.dlogp = pat(R); p.dvalue = pat(R); p.macc = p.macc0; o.ppo_loss(x, p.pp, R, p.dlogp, p.dvalue, p.macc, p.part);
  if (p.part == 3) {
    std::vector<double> m = p.macc0; p.dlogp1 = pat(R); p.dvalue1 = pat(R); o.ppo_loss(x, p.pp, R, p.dlogp1, p.dvalue1, m, 1);
    p.dlogp2 = pat(R); p.dvalue2 = pat(R); o.ppo_loss(x, p.pp, R, p.dlogp2, p.dvalue2, m, 2);
  }
}
static Chk check_loss(const Loss& p) {
  Chk k; const int R = p.R; double m[5] = {0, 0, 0, 0, 0}, e[5] = {0, 0, 0, 0, 0}, ab[5] = {0, 0, 0, 0, 0};
  if (p.chained) { double s[2]; own_stats(p, s); k.upd("stats", std::fabs(p.stats_seen[0] - s[0]), gamma_d(R + 2) * std::fabs(s[0]) + gamma_d(R + 2) * 0.7 * (1 + p.ratio) * R, 0, 0); k.upd("stats", std::fabs(p.stats_seen[1] - s[1]), gamma_d(R + 2) * s[1], 0, 1); }
  for (int r = 0; r < R; ++r) {
    if (p.part & 1) {
      const PolRef a = policy_ref(p.pp, R, p.stats_seen.data(), p.x.adv[r], p.x.logp[r], p.x.logp_old[r]);
      if (a.zero && R > 1) k.exact("zero", p.dlogp[r], 0.0f, r, 0); else k.upd("dlogp", std::fabs(p.dlogp[r] - a.dlogp), SECOND_ORDER * a.e_dlogp, r, 0);
      m[0] -= a.surr; e[0] += a.e_surr; ab[0] += std::fabs(a.surr); m[2] += p.x.ent[r]; ab[2] += std::fabs(p.x.ent[r]); m[3] += a.clipfrac; m[4] -= a.d; e[4] += a.e_d; ab[4] += std::fabs(a.d);
    } else k.exact("untouched", p.dlogp[r], PATTERN, r, 0);
    if (p.part & 2) {
      const ValRef b = value_ref(p.pp, p.x.value[r], 0, p.x.value_old[r], p.x.target[r]); const double dv = (double)p.pp.vcoef / R * b.gv;
      if (b.zero) k.exact("zero", p.dvalue[r], 0.0f, r, 1); else k.upd("dvalue", std::fabs(p.dvalue[r] - dv), SECOND_ORDER * ((double)p.pp.vcoef / R * b.e_gv + 3 * U * std::fabs(dv)), r, 1);
      m[1] += b.m1; e[1] += b.e_m1 + U * b.m1; ab[1] += b.m1;
    } else k.exact("untouched", p.dvalue[r], PATTERN, r, 1);
  }
  for (int i = 0; i < 8; ++i) {
    const bool on = i < 5 && (i == 1 ? (p.part & 2) : (p.part & 1));
    if (!on) k.exact("untouched", p.macc[i], p.macc0[i], i, 2);
    else k.upd("macc", std::fabs(p.macc[i] - (p.macc0[i] + m[i])), SECOND_ORDER * (e[i] + gamma_d(R + 16) * (ab[i] + std::fabs(p.macc0[i]))) + (i == 3 ? 1e-9 : 0.0), i, 2);
  }
  if (p.part == 3) {
    if (p.dlogp1.size() != (size_t)R) k.fail("links", "half launches missing");
    else { k.same("links", p.dlogp1, p.dlogp); k.same("links", p.dvalue2, p.dvalue); k.same("untouched", p.dvalue1, pat(R)); k.same("untouched", p.dlogp2, pat(R)); }
  }
  return k;
}
static void loss_case(int R, int part, int ratio, bool foreign, bool chained, const char* ppn, PpoParams pp) {
  Loss p; p.R = R; p.part = part; p.ratio = ratio; p.foreign = foreign; p.chained = chained; p.pp = pp; make_loss(p, next_id++);
  char what[140]; snprintf(what, sizeof what, "R=%d part=%d ratio=%d stats=%s pp=%s", R, part, ratio, foreign ? "foreign" : (chained ? "adv_stats" : "own"), ppn);
  char live[260]; snprintf(live, sizeof live, " live in %.3f zero %.3f taken %.3f lr %.3f vi %.3f va %.3f vz %.3f redraws %d margin_violations %ld", p.share[0], p.share[1], p.share[2], p.share[3], p.share[4], p.share[5], p.share[6], p.redraws, p.viol);
  bool ok = p.viol == 0; if (R >= 255) for (int i = 0; i < 7; ++i) ok = ok && p.share[i] >= 0.05;
  const Muts muts{{M_PART, part != 3}, {M_STATS11, foreign && (part & 1)}, {M_FP32_200, ratio == 200 && (part & 1) && R > 1}, {M_CLIP_D, R >= 255 && (part & 1)}, {M_VZERO, R >= 255 && (part & 2)},
                  {M_VCOEF, (part & 2) != 0}, {M_INV, (part & 2) || ((part & 1) && R > 1)}};
  run_case("ppo_loss", what, muts, [&](Ops& o) { run_loss(p, o); }, [&]() { return check_loss(p); }, live, ok);
}

// adv_stats / sumsq: double sums, atomic and deterministic forms
struct Sums { bool sq = false, det = false; int R = 0, ratio = 0, nb = 0, w = 0; float scale = 1; std::vector<float> x; std::vector<double> o, o0, part, part2, red, red0; bool order_distinct = false, order_demanded = false; };
static double term(const Sums& p, size_t i, int col) { const double v = p.sq ? (double)p.x[i] * p.scale : (double)p.x[i]; return (p.sq || col == 1) ? v * v : v; }
static void run_sums(Sums& p, Ops& o) {
  p.o = p.o0; p.part = p.det ? patd((size_t)p.nb * p.w + 8) : std::vector<double>();   // 8 words behind the partials: they stay the pattern
  auto go = [&](std::vector<double>& out, std::vector<double>& part) { if (p.sq) o.sumsq(p.x, p.scale, out, part); else o.adv_stats(p.x, p.R, out, part); };
  go(p.o, p.part);
  if (p.det) { std::vector<double> o2 = p.o0; p.part2 = patd((size_t)p.nb * p.w + 8); go(o2, p.part2); p.red = p.red0; std::vector<double> pp(p.part.begin(), p.part.begin() + (size_t)p.nb * p.w); o.reduce_double(pp, p.nb, p.w, p.red); }
}
static Chk check_sums(Sums& p) {
  Chk k; const size_t n = p.x.size(); const int nb = p.nb, w = p.w;
  if (!p.det) {
    for (int c = 0; c < w; ++c) { double s = 0, a = 0; for (size_t i = 0; i < n; ++i) { s += term(p, i, c); a += std::fabs(term(p, i, c)); } k.upd("sum", std::fabs(p.o[c] - (p.o0[c] + s)), gamma_d((double)n + nb + 2) * (a + std::fabs(p.o0[c])), 0, c); }
    for (size_t c = w; c < p.o.size(); ++c) k.exact("untouched", p.o[c], p.o0[c], 0, (long)c);
    return k;
  }
  k.same("untouched", p.o, p.o0);
  for (int b = 0; b < nb; ++b) for (int c = 0; c < w; ++c) {
    double s = 0, a = 0; size_t cnt = 0; for (size_t i = (size_t)b * 256; i < n; i += (size_t)nb * 256) for (size_t t = 0; t < 256 && i + t < n; ++t) { s += term(p, i + t, c); a += std::fabs(term(p, i + t, c)); ++cnt; }
    if (cnt == 0) k.exact("empty_block", p.part[(size_t)b * w + c], 0.0, b, c); else k.upd("partial", std::fabs(p.part[(size_t)b * w + c] - s), gamma_d((double)cnt + 2) * a, b, c);
  }
  for (int i = 0; i < 8; ++i) k.exact("untouched", p.part[(size_t)nb * w + i], pattern<double>(), nb, i);
  k.same("relaunch", p.part2, p.part);
  if (p.red.size() != p.red0.size()) { k.fail("reduce", "missing"); return k; }
  p.order_distinct = false;
  for (int c = 0; c < w; ++c) { k.exact("reduce", p.red[c], p.red0[c] + chain(p.part.data() + c, (size_t)nb, (size_t)w), 0, c); if (!same_bits(chain(p.part.data() + c, (size_t)nb, (size_t)w), tree(p.part.data() + c, (size_t)nb, (size_t)w))) p.order_distinct = true; }
  return k;
}
static void sums_case(bool sq, bool det, int n, int ratio, float scale, const char* scn) {
  Sums p; p.sq = sq; p.det = det; p.R = n; p.ratio = ratio; p.scale = scale; p.nb = sq ? SUMSQ_BLOCKS : ADV_STATS_BLOCKS; p.w = sq ? 1 : 2; const uint32_t tag = 0x53000000u + 16u * next_id++;
  p.o0.assign(sq ? 1 : 16, 0.0); for (size_t i = p.w; i < p.o0.size(); ++i) p.o0[i] = pattern<double>();
  p.red0.assign(p.w, 0.0); for (int c = 0; c < p.w; ++c) p.red0[c] = 0.37 + c;
  char what[140]; if (sq) snprintf(what, sizeof what, "n=%d scale=%s form=%s", n, scn, det ? "part" : "atomic"); else snprintf(what, sizeof what, "R=%d ratio=%d form=%s", n, ratio, det ? "part" : "atomic");
  p.order_demanded = det && n > 4 * 256 * 4;   // at least four blocks with a few hundred elements each
  // double sums of fp32 data are often exact, and then every order gives the same bits: where the order is demanded, the family's salt is the first
  // whose partials (of the host model) a balanced tree adds to other bits than the chain
  for (uint32_t salt = 0; salt < 16; ++salt) {
    p.x.resize(n); for (int i = 0; i < n; ++i) p.x[i] = 0.7f * (hv(tag, i, salt) + (float)ratio * 0.57735027f);
    if (!p.order_demanded) break;
    Ops h; run_sums(p, h); check_sums(p); if (p.order_distinct) break;
  }
  run_case(sq ? "sumsq" : "adv_stats", what, sq ? Muts{{M_SS_SCALE, scale != 1.0f}} : Muts{}, [&](Ops& o) { run_sums(p, o); }, [&]() {
    Chk k = check_sums(p); if (p.order_demanded && !p.order_distinct) k.fail("order", "a balanced tree over the partials gives the same bits as the chain"); return k; },
    p.order_demanded ? " order=distinct" : (det ? " order=n/a" : ""));
}

// critic head
struct Critic { int H = 0, R = 0; PpoParams pp{}; std::vector<float> h, w, b, vo, tg, value, dvalue, dout, dh, out40, value2, dvalue2, unused; std::vector<double> macc, macc0, vref, e_v; int redraws = 0; long viol = 0; double share[3] = {0, 0, 0}; };
static void make_critic(Critic& p, uint32_t id) {
  const uint32_t tag = 0x54000000u + 32u * id; const int H = p.H, R = p.R;
  fill(p.h, (size_t)R * H, tag, 1.0f); fill(p.w, H, tag + 1, 1.0f / std::sqrt((float)H)); fill(p.b, 1, tag + 2, 0.25f, 0.5f); p.vo.resize(R); p.tg.resize(R); p.vref.resize(R); p.e_v.resize(R);
  for (int r = 0; r < R; ++r) {
    double s = p.b[0], a = std::fabs(s); for (int k = 0; k < H; ++k) { const double q = (double)p.h[(size_t)r * H + k] * p.w[k]; s += q; a += std::fabs(q); }
    p.vref[r] = s; p.e_v[r] = gamma_n(2 * (H / 64) + 7) * a;
    for (uint32_t salt = 0;; ++salt) { draw_value(p.pp, tag, r, salt, s, p.vo[r], p.tg[r]); if (value_ref(p.pp, s, p.e_v[r], p.vo[r], p.tg[r]).margin > MARGIN) break; ++p.redraws; }
    const ValRef v = value_ref(p.pp, s, p.e_v[r], p.vo[r], p.tg[r]); p.viol += !(v.margin > MARGIN); p.share[v.outcome] += 1.0 / R;
  }
  p.macc0.resize(8); for (int i = 0; i < 8; ++i) p.macc0[i] = 2.5 + 0.25 * i;
}
static void run_critic(Critic& p, Ops& o) {
  const int R = p.R, H = p.H;
  p.value = pat(R); p.dvalue = pat(R); p.dout = pat((size_t)R * 40); p.dh = pat((size_t)R * H); p.macc = p.macc0;
  o.critic_head(H, p.h, p.w, p.b, p.vo, p.tg, p.pp, R, p.value, p.dvalue, p.dout, p.dh, p.macc);
  // the unfused path on the same inputs: the output GEMM's result (here: the double dot product rounded once) in column 0 of an ld = 40 array
  p.out40.assign((size_t)R * 40, QNAN); for (int r = 0; r < R; ++r) p.out40[(size_t)r * 40] = (float)p.vref[r];
  p.value2 = pat(R); o.critic_value(p.out40, 40, R, p.value2);
  Ops::LossIO x; x.value = p.value2; x.value_old = p.vo; x.target = p.tg; x.stats.assign(16, 0.0);   // the policy half's inputs stay null: part = 2 may not read them
  p.dvalue2 = pat(R); p.unused = pat(R); std::vector<double> m = p.macc0; o.ppo_loss(x, p.pp, R, p.unused, p.dvalue2, m, 2);
}
static Chk check_critic(const Critic& p) {
  Chk k; const int R = p.R, H = p.H; double m1 = 0, e1 = 0;
  for (int r = 0; r < R; ++r) {
    k.upd("value", std::fabs(p.value[r] - p.vref[r]), p.e_v[r], r, 0);
    const ValRef v = value_ref(p.pp, p.value[r], 0, p.vo[r], p.tg[r]), v2 = value_ref(p.pp, p.value2[r], 0, p.vo[r], p.tg[r]); const double c = (double)p.pp.vcoef / R, dv = c * v.gv;
    if (v.zero) k.exact("zero", p.dvalue[r], 0.0f, r, 1); else k.upd("dvalue", std::fabs(p.dvalue[r] - dv), SECOND_ORDER * (c * v.e_gv + 3 * U * std::fabs(dv)), r, 1);
    m1 += v.m1; e1 += v.e_m1 + U * v.m1;
    for (int j = 0; j < H; ++j) { volatile float f = p.dvalue[r] * p.w[j]; k.exact("dh", p.dh[(size_t)r * H + j], (float)f, r, j); }
    k.exact("dout", p.dout[(size_t)r * 40], p.dvalue[r], r, 0); for (int c2 = 1; c2 < 40; ++c2) k.exact("untouched", p.dout[(size_t)r * 40 + c2], PATTERN, r, c2);
    // the unfused path: the same branch, and values within the sum of the two bounds
    k.exact("unfused", p.value2[r], (float)p.vref[r], r, 2);
    if (v.outcome != v2.outcome || (p.dvalue[r] == 0.0f) != (p.dvalue2[r] == 0.0f)) k.fail("unfused", "another branch of the value loss");
    k.upd("unfused", std::fabs(p.value[r] - p.value2[r]), p.e_v[r] + U * std::fabs(p.vref[r]), r, 3);
    k.upd("unfused", std::fabs(p.dvalue[r] - p.dvalue2[r]), SECOND_ORDER * (c * (v.e_gv + v2.e_gv + p.e_v[r] + U * std::fabs(p.vref[r])) + 6 * U * std::fabs(dv)), r, 4);
  }
  for (int i = 0; i < 8; ++i) if (i == 1) k.upd("macc", std::fabs(p.macc[1] - (p.macc0[1] + m1)), SECOND_ORDER * (e1 + gamma_d(R + 16) * (m1 + p.macc0[1])), 1, 0); else k.exact("untouched", p.macc[i], p.macc0[i], i, 0);
  k.same("untouched", p.unused, pat(R));
  return k;
}
static void critic_case(int H, int R) {
  Critic p; p.H = H; p.R = R; p.pp = default_pp(); make_critic(p, next_id++);
  char what[120]; snprintf(what, sizeof what, "H=%d R=%d", H, R);
  char live[200]; snprintf(live, sizeof live, " live vi %.3f va %.3f vz %.3f redraws %d margin_violations %ld", p.share[0], p.share[1], p.share[2], p.redraws, p.viol);
  bool ok = p.viol == 0; if (R >= 255) for (int i = 0; i < 3; ++i) ok = ok && p.share[i] >= 0.05;
  run_case("critic_head", what, Muts{{M_VZERO, R >= 255}, {M_VCOEF, true}, {M_INV, true}, {M_CH_BIAS, true}, {M_CH_DH, R > 1}, {M_CH_DOUT, true}}, [&](Ops& o) { run_critic(p, o); }, [&]() { return check_critic(p); }, live, ok);
}
static void mirror_loss_case(int R, int part) {
  const uint32_t tag = 0x55000000u + 16u * next_id++; const float sa = 1.0f, sc = 0.01f; const size_t RJ = (size_t)R * KBJ_NU;
  char what[120]; snprintf(what, sizeof what, "R=%d part=%d", R, part);
  std::vector<float> y, ym, v, vm, dv0, dy, dym, dvalue, dvm; std::vector<double> macc0(8), macc; for (int i = 0; i < 8; ++i) macc0[i] = 0.75 + 0.5 * i;
  fill(y, RJ, tag, 1.0f); fill(ym, RJ, tag + 1, 1.0f); fill(v, R, tag + 2, 2.0f); fill(vm, R, tag + 3, 2.0f); fill(dv0, R, tag + 4, 1.0f / R);
  auto run = [&](Ops& o) { dy = pat(RJ); dym = pat(RJ); dvalue = dv0; dvm = pat(R); macc = macc0; o.mirror_loss(y, ym, v, vm, sa, sc, R, dy, dym, dvalue, dvm, macc, part); };
  auto check = [&]() {
    Chk k; double m5 = 0, e5 = 0, m6 = 0, e6 = 0; const double ca = (double)sa / (20.0 * R);
    for (int r = 0; r < R; ++r) {
      double la = 0;
      for (int i = 0; i < KBJ_NU; ++i) {
        const int s = i < 5 ? i + 5 : (i < 10 ? i - 5 : i); const size_t a = (size_t)r * KBJ_NU + i, b = (size_t)r * KBJ_NU + s; const double e = (double)y[a] + ym[b], g = 2 * ca * e;
        if (part & 1) { k.upd("dy", std::fabs(dy[a] - g), SECOND_ORDER * 3 * U * std::fabs(g), r, i); k.upd("dym", std::fabs(dym[b] - g), SECOND_ORDER * 3 * U * std::fabs(g), r, s); la += e * e; }
        else { k.exact("untouched", dy[a], PATTERN, r, i); k.exact("untouched", dym[b], PATTERN, r, s); }
      }
      m5 += sa * la / 20.0; e5 += sa * la / 20.0 * (gamma_n(KBJ_NU + 3) + 2 * U);
      const double ev = (double)v[r] - vm[r], gv = 2.0 * sc / R * ev;
      if (part & 2) { k.upd("dvalue", std::fabs(dvalue[r] - (dv0[r] + gv)), SECOND_ORDER * (3 * U * std::fabs(gv) + U * std::fabs(dv0[r] + gv)), r, 0); k.upd("dvalue_m", std::fabs(dvm[r] + gv), SECOND_ORDER * 3 * U * std::fabs(gv), r, 1); m6 += sc * ev * ev; e6 += 4 * U * sc * ev * ev; }
      else { k.exact("untouched", dvalue[r], dv0[r], r, 0); k.exact("untouched", dvm[r], PATTERN, r, 1); }
    }
    for (int i = 0; i < 8; ++i) {
      if (i == 5 && (part & 1)) k.upd("macc", std::fabs(macc[5] - (macc0[5] + m5)), SECOND_ORDER * (e5 + gamma_d(R + 2) * (m5 + macc0[5])), 5, 0);
      else if (i == 6 && (part & 2)) k.upd("macc", std::fabs(macc[6] - (macc0[6] + m6)), SECOND_ORDER * (e6 + gamma_d(R + 2) * (m6 + macc0[6])), 6, 0);
      else k.exact("untouched", macc[i], macc0[i], i, 0);
    }
    return k;
  };
  run_case("mirror_loss", what, Muts{{M_MIR_MAP, (part & 1) != 0}, {M_MIR_SIGN, (part & 1) != 0}, {M_PART, part != 3}}, run, check);
}
static void metrics_case(int R, int kind) {   // kind 0: own statistics, 1: caller's (stats[11] > 0), 2: a variance that rounding made negative
  static const char* KN[3] = {"own", "foreign", "negative_var"}; char what[120]; snprintf(what, sizeof what, "R=%d stats=%s", R, KN[kind]);
  const PpoParams pp = default_pp(); std::vector<double> macc(8), stats(16, 0.0); std::vector<float> m;
  for (int i = 0; i < 8; ++i) macc[i] = (i % 2 ? -1.0 : 1.0) * R * (0.3 + 0.17 * i);
  const double cnt = kind == 1 ? 4.0 * R : (double)R, mean = 0.37; stats[11] = kind == 1 ? cnt : 0.0; stats[0] = cnt * mean; stats[1] = cnt * (kind == 2 ? mean * mean * (1.0 - 1e-12) : mean * mean + 0.25);
  auto run = [&](Ops& o) { m = pat(10); o.metrics(macc, stats, pp, R, m); };
  auto check = [&]() {
    Chk k; const double pol = macc[0] / R, vl = macc[1] / R, en = macc[2] / R, ma = macc[5] / R, mc = macc[6] / R, mu = stats[0] / cnt, var = stats[1] / cnt - mu * mu;
    const double ref[10] = {pol + pp.vcoef * vl - pp.ecoef * en + ma + mc, pol, vl, en, macc[3] / R, macc[4] / R, mu, std::sqrt(var > 0 ? var : 0), ma, mc};
    const double mag0 = std::fabs(pol) + std::fabs(pp.vcoef * vl) + std::fabs(pp.ecoef * en) + std::fabs(ma) + std::fabs(mc);
    for (int i = 0; i < 10; ++i) {
      if (i == 7 && kind == 2) { k.exact("adv_std", m[7], 0.0f, 7, 0); continue; }
      k.upd("metric", std::fabs(m[i] - ref[i]), U * std::fabs(ref[i]) + 8 * UD * (i == 0 ? mag0 : (i == 7 ? (mu * mu + 0.25) / std::sqrt(0.25) : std::fabs(ref[i]))), i, 0);
    }
    return k;
  };
  run_case("ppo_metrics", what, Muts{}, run, check);
}

// ---- group D -------------------------------------------------------------------------------------------------------------------------------
static void matvec_case(int M, int K, bool add) {
  const uint32_t tag = 0x60000000u + 16u * next_id++; char what[120]; snprintf(what, sizeof what, "M=%d K=%d add=%d", M, K, add);
  std::vector<float> W, x, a, y; fill(W, (size_t)M * K, tag, 1.0f / std::sqrt((float)K)); fill(x, K, tag + 1, 1.0f); if (add) fill(a, M, tag + 2, 0.5f);
  auto run = [&](Ops& o) { y = pat(M); o.matvec(W, x, a, M, K, y); };
  auto check = [&]() { Chk k; for (int m = 0; m < M; ++m) { double s = add ? a[m] : 0.0, ab = std::fabs(s); for (int c = 0; c < K; ++c) { const double q = (double)W[(size_t)m * K + c] * x[c]; s += q; ab += std::fabs(q); } k.upd("y", std::fabs(y[m] - s), gamma_n(2 * ((K + 63) / 64) + 7) * ab, m, 0); } return k; };
  run_case("matvec", what, Muts{}, run, check);
}
static void matvec_t_case(int K, int N, bool det) {
  const uint32_t tag = 0x61000000u + 16u * next_id++; char what[120]; snprintf(what, sizeof what, "K=%d N=%d form=%s", K, N, det ? "part" : "atomic");
  std::vector<float> W, x, y0, y, part, part2, red; fill(W, (size_t)K * N, tag, 1.0f / std::sqrt((float)K)); fill(x, K, tag + 1, 1.0f); fill(y0, N, tag + 2, 0.5f);
  const int S = MATVEC_T_SLICES; bool distinct = false;
  auto run = [&](Ops& o) {
    y = y0; part = det ? pat((size_t)S * N) : std::vector<float>(); o.matvec_t(W, x, K, N, y, part);
    if (det) { std::vector<float> y2 = y0; part2 = pat((size_t)S * N); o.matvec_t(W, x, K, N, y2, part2); red = y0; o.reduce_rows(part, S, N, red); }
  };
  auto check = [&]() {
    Chk k; const int per = (K + 63) / 64;
    for (int n = 0; n < N; ++n) {
      double tot = 0, tab = 0;
      for (int by = 0; by < S; ++by) {
        double s = 0, ab = 0; for (int j = 4 * by; j < K; j += 4 * S) for (int ph = 0; ph < 4 && j + ph < K; ++ph) { const double q = (double)W[(size_t)(j + ph) * N + n] * x[j + ph]; s += q; ab += std::fabs(q); }
        tot += s; tab += ab;
        if (det) k.upd("partial", std::fabs(part[(size_t)by * N + n] - s), gamma_n(2 * per + 3) * ab, by, n);
      }
      if (!det) k.upd("y", std::fabs(y[n] - (y0[n] + tot)), gamma_n(2 * per + 3 + S + 1) * (tab + std::fabs(y0[n])), 0, n);
      else { k.exact("untouched", y[n], y0[n], 0, n); k.exact("reduce", red[n], y0[n] + chain(part.data() + n, (size_t)S, (size_t)N), 0, n); if (!same_bits(chain(part.data() + n, (size_t)S, (size_t)N), tree(part.data() + n, (size_t)S, (size_t)N))) distinct = true; }
    }
    if (det) { k.same("relaunch", part2, part); if (K >= 64 && !distinct) k.fail("order", "a balanced tree over the partials gives the same bits as the chain"); }
    return k;
  };
  run_case("matvec_t_acc", what, Muts{}, run, check, det ? (K >= 64 ? " order=distinct" : " order=n/a") : "");   // K < 64: at most two partial rows are non-zero
}
static void outer_case(int M, int N) {
  const uint32_t tag = 0x62000000u + 16u * next_id++; char what[120]; snprintf(what, sizeof what, "M=%d N=%d", M, N);
  std::vector<float> C0, C, u, v; fill(C0, (size_t)M * N, tag, 1.0f); fill(u, M, tag + 1, 1.0f); fill(v, N, tag + 2, 1.0f);
  auto run = [&](Ops& o) { C = C0; o.outer_acc(C, u, v, M, N); };
  auto check = [&]() { Chk k; for (int m = 0; m < M; ++m) for (int n = 0; n < N; ++n) { const size_t i = (size_t)m * N + n; const double q = (double)u[m] * v[n]; k.upd("C", std::fabs(C[i] - (C0[i] + q)), SECOND_ORDER * U * (2 * std::fabs(q) + std::fabs(C0[i])), m, n); } return k; };
  run_case("outer_acc", what, Muts{}, run, check);
}
static void colsum_case(int M, int N, int ld, bool det) {
  const uint32_t tag = 0x63000000u + 16u * next_id++; char what[120]; snprintf(what, sizeof what, "M=%d N=%d ld=%d form=%s", M, N, ld, det ? "part" : "atomic");
  std::vector<float> X, o0, out, part, part2, red; fill(X, (size_t)M * ld, tag, 1.0f); fill(o0, N, tag + 1, 0.5f);
  for (int m = 0; m < M; ++m) for (int c = N; c < ld; ++c) X[(size_t)m * ld + c] = QNAN;
  bool distinct = false; const bool demanded = det && M >= 2047;
  auto run = [&](Ops& o) {
    out = o0; part = det ? pat((size_t)DETP_ROWS * N) : std::vector<float>(); o.colsum(X, M, N, ld, out, part);
    if (det) { std::vector<float> o2 = o0; part2 = pat((size_t)DETP_ROWS * N); o.colsum(X, M, N, ld, o2, part2); red = o0; o.reduce_rows(part, DETP_ROWS, N, red); }
  };
  auto check = [&]() {
    Chk k;
    for (int c = 0; c < N; ++c) {
      if (!det) { double s = 0, ab = 0; for (int m = 0; m < M; ++m) { s += X[(size_t)m * ld + c]; ab += std::fabs(X[(size_t)m * ld + c]); } k.upd("sum", std::fabs(out[c] - (o0[c] + s)), gamma_n((M + 2047) / 2048 + 3 + DETP_ROWS + 1) * (ab + std::fabs(o0[c])), 0, c); continue; }
      for (int by = 0; by < DETP_ROWS; ++by) {   // additions only: the kernel's order, bit for bit (a row slice that owns no row of X gives +0.0)
        float p[4]; for (int ph = 0; ph < 4; ++ph) { p[ph] = 0; for (int m = ph + 4 * by; m < M; m += 4 * DETP_ROWS) p[ph] += X[(size_t)m * ld + c]; }
        k.exact("partial", part[(size_t)by * N + c], ((p[0] + p[1]) + p[2]) + p[3], by, c);
      }
      k.exact("untouched", out[c], o0[c], 0, c); k.exact("reduce", red[c], o0[c] + chain(part.data() + c, (size_t)DETP_ROWS, (size_t)N), 0, c);
      if (!same_bits(chain(part.data() + c, (size_t)DETP_ROWS, (size_t)N), tree(part.data() + c, (size_t)DETP_ROWS, (size_t)N))) distinct = true;
    }
    if (det) { k.same("relaunch", part2, part); if (demanded && !distinct) k.fail("order", "a balanced tree over the partials gives the same bits as the chain"); }
    return k;
  };
  run_case("colsum", what, Muts{{M_CS_PHASE, M > 3}, {M_CS_LD, ld != N && M > 1}}, run, check, demanded ? " order=distinct" : (det ? " order=n/a" : ""));
}

int main(int argc, char** argv) {
  tally.args(argc, argv);
  if (!tally.plan_mode) arena.init();
  // ---- A
  for (int T : {1, 3}) for (int N : {5, 70}) for (int B : {1, 5, 33, 64}) if (B <= N) for (int sc = 0; sc < 2; ++sc) gather_rows_case(T, N, B, 68, 68, 68, sc != 0, false);
  for (int w : {72, 476}) for (int B : {33, 64}) for (int sc = 0; sc < 2; ++sc) gather_rows_case(3, 70, B, w, w, w, sc != 0, false);
  for (int sc = 0; sc < 2; ++sc) { gather_rows_case(3, 70, 33, 68, 476, 72, sc != 0, false); gather_rows_case(3, 70, 33, 68, 68, 68, sc != 0, true); }
  for (int shape = 0; shape < 2; ++shape) for (int nulls = 0; nulls < 2; ++nulls) { const int T = shape ? 1 : 3, N = shape ? 5 : 70, B = shape ? 5 : 33;
    gather_small_case(T, N, B, KBJ_NU + 4, KBJ_NU + 5, nulls != 0); gather_small_case(T, N, B, 0, KBJ_NU + 4, nulls != 0); gather_small_case(T, N, B, 0, KBJ_NU + 5, nulls != 0); }
  for (int np : {4, 16}) for (int nl : {0, 2}) for (int H : {64, 192, 512}) for (int B : {1, 33}) gather_carry_case(np, nl, H, B);
  for (int critic = 0; critic < 2; ++critic) for (int rows : {1, 33}) mirror_rows_case(critic != 0, rows);
  repitch_rows_case(64, 475, 476); repitch_rows_case(3, 5, 8);
  repitch_pad_case(33, 65, 68); repitch_pad_case(33, 68, 68); repitch_pad_case(33, 72, 68);
  // ---- B: each axis swept at one or two settings of the others
  { const HeadParams d = default_hp(68);
    for (int T : {1, 9, 10, 11, 19, 20, 21, 30}) for (int B : {3, 33}) headb_case(T, B, 68, "default", d, K_HASH, false, false, false, T == 21 && B == 33);
    for (int T : {11, 21}) for (int B : {1, 4}) headb_case(T, B, 68, "default", d, K_HASH, false, false, false, false);
    headb_case(11, 33, 72, "default", default_hp(72), K_HASH, false, false, false, false);
    HeadParams h;
    h = d; h.max_std = 0.35f; headb_case(21, 33, 68, "max_std=0.35", h, K_HASH, false, false, false, true);
    h = d; h.min_std = 0.2f; headb_case(21, 33, 68, "min_std=0.2", h, K_HASH, false, false, false, true);
    h = d; h.var_scale = 1.5f; headb_case(21, 33, 68, "var_scale=1.5", h, K_HASH, false, false, false, true);
    h = d; h.var_scale = 0.25f; headb_case(21, 33, 68, "var_scale=0.25", h, K_HASH, false, false, false, true);
    h = d; h.alpha = 1.0f; headb_case(21, 33, 68, "lpf_alpha=1", h, K_HASH, false, false, false, true);
    h = d; h.alpha = 0.1f; headb_case(21, 33, 68, "lpf_alpha=0.1", h, K_HASH, false, false, false, true);
    for (int kp : {K_NONE, K_ALL, K_SINGLE}) for (int T : {11, 21}) headb_case(T, 33, 68, "default", d, kp, false, false, false, false);
    headb_case(11, 33, 68, "default", d, K_HASH, true, false, false, false); headb_case(11, 33, 68, "default", d, K_HASH, false, true, false, false);
    for (int T : {11, 21}) headb_case(T, 33, 68, "default", d, K_HASH, false, false, true, false); }
  // ---- C
  for (int det = 0; det < 2; ++det) for (int R : {1, 255, 256, 257, 8191, 8192, 8193, 20000}) sums_case(false, det != 0, R, 0, 1.0f, "");
  for (int det = 0; det < 2; ++det) for (int ratio : {7, 9, 200}) sums_case(false, det != 0, 20000, ratio, 1.0f, "");
  { const PpoParams d = default_pp();
    for (int R : {1, 255, 256, 257, 1000}) for (int part = 0; part < 4; ++part) loss_case(R, part, 0, false, false, "default", d);
    for (int ratio : {0, 7, 9, 200}) { loss_case(1000, 3, ratio, false, true, "default", d); loss_case(1000, 3, ratio, true, false, "default", d); }
    PpoParams q;
    q = d; q.ecoef = 0.5f; loss_case(257, 3, 0, false, false, "entropy_coef=0.5", q);
    q = d; q.vcoef = 2.0f; loss_case(257, 3, 0, false, false, "value_loss_coef=2", q);
    q = d; q.clip = 0.05f; loss_case(257, 3, 0, false, false, "clip_param=0.05", q);
    q = d; q.clip = 0.6f; loss_case(257, 3, 0, false, false, "clip_param=0.6", q);
    q = d; q.vclip = 0.05f; loss_case(257, 3, 0, false, false, "value_clip=0.05", q);
    q = d; q.vclip = 5.0f; loss_case(257, 3, 0, false, false, "value_clip=5", q);
    q = d; q.lrclip = 0.25f; loss_case(257, 3, 0, false, false, "log_ratio_clip=0.25", q);
    q = d; q.adv_eps = 0.5f; loss_case(257, 3, 0, false, false, "adv_eps=0.5", q);
    q = PpoParams{0.1f, 0.1f, 1.5f, 0.1f, 0.4f, 0.1f}; loss_case(257, 3, 0, false, false, "combined", q); }
  for (int H = 64; H <= 512; H += 64) for (int R : {1, 3, 4, 5, 100}) critic_case(H, R);
  for (int H : {64, 512}) for (int R : {8192, 8193, 8200}) critic_case(H, R);
  for (int R : {1, 257}) for (int part = 1; part < 4; ++part) mirror_loss_case(R, part);
  for (int R : {1, 1000}) for (int kind = 0; kind < 3; ++kind) metrics_case(R, kind);
  // ---- D
  for (int H = 64; H <= 512; H += 64) matvec_case(4 * H, H, true);
  for (int add = 0; add < 2; ++add) { matvec_case(5, 65, add != 0); matvec_case(1, 1, add != 0); }
  for (int det = 0; det < 2; ++det) { for (int H : {64, 192, 512}) matvec_t_case(4 * H, H, det != 0); matvec_t_case(7, 65, det != 0); }
  outer_case(256, 64); outer_case(2048, 512); outer_case(3, 5);
  for (int det = 0; det < 2; ++det) {
    for (int M : {1, 3, 2047, 2048, 2049, 5000}) colsum_case(M, 40, 40, det != 0);
    for (int N : {1, 64, 65, 256}) for (int pad = 0; pad < 2; ++pad) colsum_case(2049, N, pad ? N + 3 : N, det != 0);
    colsum_case(5000, 1, 40, det != 0); colsum_case(3, 40, 43, det != 0);
  }
  for (int det = 0; det < 2; ++det) for (int n : {1, 255, 256, 257, 131071, 131072, 131073, 300000}) sums_case(true, det != 0, n, 0, 1.0f, "1");
  for (int det = 0; det < 2; ++det) { sums_case(true, det != 0, 131073, 0, 0.125f, "0.125"); sums_case(true, det != 0, 131073, 0, 1.0f / 3.0f, "1/3"); }
  for (auto& kc : case_count) printf("kernel %-12s cases %d\n", kc.first.c_str(), kc.second);
  if (!tally.plan_mode) for (auto& kv : worst_frac) { printf("worst fraction of the bound, %-12s:", kv.first.c_str()); for (auto& c : kv.second) printf(" %s %.3f", c.first.c_str(), c.second); printf("\n"); }
  return tally.finish("UPDATE");
}
