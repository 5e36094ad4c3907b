"""GPU parity tests of the update path at NON-default hyperparameters: every scalar the kernels read as PpoParams / HeadParams / AdamParams and
gamma / lambda (user fields of the reference config, train.py:1763-1770, 1320-1322, 95-102) against the torch CPU oracle (oracle/nn.py, which
reads the same kbj_config fields), with the bounds of tests/test_gpu_nn.py. The other parity tests all run at layout.default_config(), where
the weight-decay term moves a parameter by 5e-10 per step, log_ratio_clip = 10 and max_std = 1 are never reached and the entropy gradient
sits under the gradient bound.

Each case comes with liveness conditions (tests/helpers.check_hparam_liveness; asserted on the CPU alone in tests/test_oracle_nn.py too):
a case whose term does not move the oracle's result by 100x the bound it is held to would test nothing."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import helpers as Hp

pytestmark = pytest.mark.gpu

_ids = lambda s: "H%d-N%d-B%d-T%d" % s


def _setup(N, B, T, H, **kw):
    import torch
    from kbot_joystick_amd.host import binding as Bd, buffers
    m = compiler.load_model("kbot-headless")
    cfg = L.default_config(num_envs=N, batch_size=B, rollout_len=T, hidden_size=H, **kw)
    ctx = Bd.Context(m, cfg, 0, torch.cuda.current_stream().cuda_stream)
    return m, cfg, ctx, torch, buffers


def _params(ctx, torch, seed=11):
    params = torch.zeros(ctx.param_count(), device="cuda:0")
    ctx.init_params(seed, params)
    ctx.synchronize()
    return params, params.detach().cpu().double()


_DEFAULT = {}


def _default_problem(shape, jb, p64):
    """The same problem under the default config on the oracle (one per shape: kbj_init_params(11) gives the same parameters every time)."""
    H, N, B, T = shape
    if shape not in _DEFAULT:
        cfg0 = L.default_config(num_envs=N, batch_size=B, rollout_len=T, hidden_size=H)
        _DEFAULT[shape] = (p64.clone(), Hp.hparam_problem(cfg0, jb, p64, Hp.synthetic_arrays(N, T, H), H, N, B))
    assert (_DEFAULT[shape][0] == p64).all()
    return _DEFAULT[shape][1]


# ---- 1. the minibatch gradient -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Hp.HPARAM_SHAPES, ids=_ids)
@pytest.mark.parametrize("name", list(Hp.HPARAM_CASES))
def test_ppo_grad_matches_autograd_under_hyperparameters(name, shape):
    """kbj_gae + kbj_ppo_grad under one non-default kbj_config against ON.gae and autograd of ON.ppo_loss(ON.ppo_variables(...)). The old
    log-probs / values are the oracle's own UNDER THE OVERRIDE plus N(0, 0.3) (with the default config's, the head cases would sit at clip
    fraction 1). Bounds as test_ppo_grad_matches_autograd: GAE 1e-5, metrics 2e-4 (1 + |x|), per leaf 2e-3 of the leaf's largest entry,
    global relative L2 1e-4.
    Measured on an MI355X over all cases x both shapes (worst): global relative L2 5.1e-6 (var_scale 0.25; 2.3e-6 without it), per leaf 1.2e-5, metrics 1.0e-6
    (1 + |x|), GAE 8.4e-7 (gamma = lam = 1)."""
    H, N, B, T = shape
    m, cfg, ctx, torch, buffers = _setup(N, B, T, H, **Hp.HPARAM_CASES[name])
    P = ctx.param_count()
    params, p64 = _params(ctx, torch)
    jb = torch.tensor(list(m.joint_bias), dtype=torch.float64)
    case = Hp.hparam_problem(cfg, jb, p64, Hp.synthetic_arrays(N, T, H), H, N, B)
    live = Hp.check_hparam_liveness(name, cfg, case, _default_problem(shape, jb, p64))
    tr = buffers.TrajBuffers(T, N, H, 2, "cuda:0")
    Hp.fill_traj(tr, case["arr"])
    ctx.gae(tr.c, tr.adv, tr.target)
    ctx.synchronize()
    e_gae = max(float((tr.adv.cpu().double() - case["adv"]).abs().max()), float((tr.target.cpu().double() - case["target"]).abs().max()))
    assert e_gae < 1e-5, (name, e_gae)
    grad, metrics = torch.zeros(P, device="cuda:0"), torch.zeros(10, device="cuda:0")
    ctx.ppo_grad(params, tr.c, case["idx"].cuda(), B, tr.adv, tr.target, grad, metrics)
    ctx.synchronize()
    e_met = Hp.check_metrics_parity(metrics.cpu().double(), case["metrics"], name)
    e_leaf, e_rel = Hp.check_grad_parity(grad.cpu().double(), case["grad"], H, label=name)
    print("hparams grad %-20s %s: rel-L2 %.2e leaf %.2e metrics %.2e gae %.2e | liveness %.2e clipfrac %.3f" % (name, _ids(shape), e_rel, e_leaf, e_met, e_gae,
                                                                                                                 live, case["metrics"]["clipfrac"]))
    ctx.close()


@pytest.mark.parametrize("shape", Hp.HPARAM_SHAPES, ids=_ids)
@pytest.mark.parametrize("mean,std", [(10.0, 0.05), (3.5, 0.5), (5.0, 0.5)], ids=["ratio200", "ratio7", "ratio10"])
def test_ppo_grad_with_advantages_far_from_zero_mean(shape, mean, std):
    """Caller-supplied advantages mean + std * randn passed straight to kbj_ppo_grad, then the same statistics through
    kbj_set_advantage_sums: same gradient and metric bounds against the fp64 oracle. E[a^2] - mean^2 in fp32 loses the variance at
    |mean| / std = 200 (ulp of 100 is 7.6e-6 against a variance of 2.5e-3). ppo_loss_kernel keeps its fp32 form, and with it every result it
    has given so far bit for bit, up to |mean| = 8 std, where that form is still good to ~6e-6 on the std, and forms mean, variance and the
    normalised advantage in double beyond, as ppo_metrics_kernel does. The cases: far beyond the switch, and on either side of it (7: the
    fp32 form near its worst conditioning; 10: the double form).
    Measured on an MI355X at ratio 200: with the fp32 variance the global relative L2 was 1.7e-3 (H 64) / 1.9e-3 (H 256) against the bound
    of 1e-4 and the test failed; in double it is 5.7e-7 / 1.4e-6 with the minibatch's own statistics and 6.6e-7 / 1.6e-6 with the caller's
    sums. At ratio 7 (fp32 form): 1.5e-6 / 2.6e-6 and 6.8e-7 / 4.2e-6; at ratio 10 (double form): 6.0e-7 / 1.5e-6 and 6.5e-7 / 1.5e-6."""
    H, N, B, T = shape
    m, cfg, ctx, torch, buffers = _setup(N, B, T, H)
    P = ctx.param_count()
    params, p64 = _params(ctx, torch)
    jb = torch.tensor(list(m.joint_bias), dtype=torch.float64)
    case = Hp.hparam_problem(cfg, jb, p64, Hp.synthetic_arrays(N, T, H), H, N, B)
    arr, idx = case["arr"], case["idx"]
    g = torch.Generator(device="cpu").manual_seed(9)
    adv = mean + std * torch.randn(T, N, generator=g)                  # float32, as the device array
    tr = buffers.TrajBuffers(T, N, H, 2, "cuda:0")
    Hp.fill_traj(tr, arr)
    ctx.gae(tr.c, tr.adv, tr.target)
    ctx.synchronize()
    tgt = tr.target.cpu()
    adv_d = adv.cuda()
    # (a) the minibatch's own statistics
    go, mt, _ = Hp.oracle_minibatch_grad(cfg, jb, p64, arr, idx, H, adv, tgt)
    assert (mt["adv_mean"] / mt["adv_std"] > 8) == (mean / std > 8) and 0.02 < mt["clipfrac"] < 0.98     # the sample is on the intended side of the switch
    grad, metrics = torch.zeros(P, device="cuda:0"), torch.zeros(10, device="cuda:0")
    ctx.ppo_grad(params, tr.c, idx.cuda(), B, adv_d, tr.target, grad, metrics)
    ctx.synchronize()
    rel_a = float((grad.cpu().double() - go).norm() / go.norm())
    print("hparams adv mean/std %g %s own statistics (sample ratio %.2f): rel-L2 %.2e" % (mean / std, _ids(shape), mt["adv_mean"] / mt["adv_std"], rel_a))
    Hp.check_metrics_parity(metrics.cpu().double(), mt, "own statistics")
    Hp.check_grad_parity(grad.cpu().double(), go, H, label="own statistics")
    # (b) the whole rollout's statistics through kbj_set_advantage_sums
    from kbot_joystick_amd.host import dist as D
    sums = D.global_advantage_sums(adv_d, 1)
    a64 = adv.double()
    go2, mt2, _ = Hp.oracle_minibatch_grad(cfg, jb, p64, arr, idx, H, adv, tgt,
                                           adv_sums=torch.stack([a64.sum(), (a64 ** 2).sum(), torch.tensor(float(a64.numel()), dtype=torch.float64)]))
    assert (mt2["adv_mean"] / mt2["adv_std"] > 8) == (mean / std > 8)
    ctx.set_advantage_sums(sums)
    g2, m2 = torch.zeros(P, device="cuda:0"), torch.zeros(10, device="cuda:0")
    ctx.ppo_grad(params, tr.c, idx.cuda(), B, adv_d, tr.target, g2, m2)
    ctx.synchronize()
    ctx.set_advantage_sums(None)
    rel_b = float((g2.cpu().double() - go2).norm() / go2.norm())
    print("hparams adv mean/std %g %s caller's sums (sample ratio %.2f):   rel-L2 %.2e" % (mean / std, _ids(shape), mt2["adv_mean"] / mt2["adv_std"], rel_b))
    Hp.check_metrics_parity(m2.cpu().double(), mt2, "caller's sums")
    Hp.check_grad_parity(g2.cpu().double(), go2, H, label="caller's sums")
    ctx.close()


# ---- 1b. the forward-only passes under the head's hyperparameters -------------------------------------------------------------------
@pytest.mark.parametrize("shape", Hp.HPARAM_SHAPES, ids=_ids)
@pytest.mark.parametrize("name", Hp.HPARAM_HEAD_CASES)
def test_ppo_forward_matches_oracle_under_head_hyperparameters(name, shape):
    """kbj_ppo_forward (actor_head_pre_kernel's clamp, actor_head_train_fwd_kernel's low-pass scan) under max_std / min_std / var_scale /
    lpf_alpha: log-probs, values, entropy with the bounds of test_ppo_forward_matches_oracle_and_gradient_pass (2e-4 / 2e-5 / 2e-4, the
    self-consistency of the returned std / mean 1e-4); action_mean and action_std element-wise against the oracle with the 2e-5 of the policy
    step's mode (the std is a <= 1.5-Lipschitz function of the same projection output, the low-pass a convex combination).
    Measured on an MI355X (worst over the cases): logp 4.1e-5 (var_scale 0.25: std ~ 0.17 sharpens the density), entropy 8.3e-6, mean 2.0e-7,
    std 1.3e-7."""
    H, N, B, T = shape
    m, cfg, ctx, torch, buffers = _setup(N, B, T, H, **Hp.HPARAM_CASES[name])
    from oracle import nn as ON
    params, p64 = _params(ctx, torch)
    jb = torch.tensor(list(m.joint_bias), dtype=torch.float64)
    arr = Hp.synthetic_arrays(N, T, H)
    g = torch.Generator(device="cpu").manual_seed(5)
    idx = torch.randperm(N, generator=g)[:B].int()
    ii = idx.long()
    arr["logp"], arr["value"], (lp, v, en) = Hp.oracle_old_policy(cfg, jb, p64, arr, H, g)
    mu, sd = Hp.oracle_head_series(ON.unflatten(p64, H), cfg, jb, arr, ii)
    if abs(cfg.max_std - 1.0) > 1e-6:
        assert 0.10 <= float((sd >= cfg.max_std).double().mean()) <= 0.90
    tr = buffers.TrajBuffers(T, N, H, 2, "cuda:0")
    Hp.fill_traj(tr, arr)
    dev = "cuda:0"
    o_lp, o_v, o_en = (torch.zeros(T, B, device=dev) for _ in range(3))
    o_sd, o_mu = torch.zeros(T, B, 20, device=dev), torch.zeros(T, B, 20, device=dev)
    ctx.ppo_forward(params, tr.c, idx.cuda(), B, o_lp, o_v, o_en, o_sd, o_mu)
    ctx.synchronize()
    e_lp, e_v, e_en = (float((a.cpu().double() - b[:, ii]).abs().max()) for a, b in ((o_lp, lp), (o_v, v), (o_en, en)))
    e_mu, e_sd = float((o_mu.cpu().double() - mu).abs().max()), float((o_sd.cpu().double() - sd).abs().max())
    print("hparams forward %-14s %s: logp %.2e value %.2e entropy %.2e mean %.2e std %.2e" % (name, _ids(shape), e_lp, e_v, e_en, e_mu, e_sd))
    assert e_lp < 2e-4 and e_v < 2e-5 and e_en < 2e-4
    assert e_mu < 2e-5 and e_sd < 2e-5
    assert float(o_sd.min()) > 0 and float(o_sd.max()) <= cfg.max_std + 1e-6
    ent = (0.5 + 0.5 * np.log(2 * np.pi) + o_sd.cpu().double().log()).sum(-1)
    assert (ent - o_en.cpu().double()).abs().max() < 1e-4
    lp2 = ON.gaussian_logp(arr["action"].double()[:, ii], o_mu.cpu().double(), o_sd.cpu().double())
    assert (lp2 - o_lp.cpu().double()).abs().max() < 1e-4
    ctx.close()


@pytest.mark.parametrize("H,N", [(64, 96), (256, 100)])
@pytest.mark.parametrize("name", Hp.HPARAM_HEAD_CASES)
def test_policy_step_matches_oracle_under_head_hyperparameters(name, H, N):
    """kbj_policy_step (actor_head_fused_kernel: clamp, low-pass, sample, log-prob) under the head's hyperparameters, bounds of
    test_policy_step_matches_oracle: mode 2e-5, log-prob of the mode 1e-4, low-pass state 1e-5, log-prob of a sample 1e-3, unit-Gaussian
    draws; and the std implied by the log-prob of the mode, sum_j log std_j = -logp - 10 log(2 pi), 1e-4.
    Measured on an MI355X (worst over the cases): mode 3.7e-7, log-prob 4.3e-6, low-pass state 3.7e-7."""
    m, cfg, ctx, torch, buffers = _setup(N, 32, 4, H, **Hp.HPARAM_CASES[name])
    from oracle import nn as ON
    params, p64 = _params(ctx, torch, seed=3)
    p = ON.unflatten(p64, H)
    jb = torch.tensor(list(m.joint_bias), dtype=torch.float64)
    g = torch.Generator(device="cpu").manual_seed(0)
    aobs = torch.zeros(N, L.LD_ACTOR); aobs[:, :65] = torch.randn(N, 65, generator=g)
    cobs = torch.zeros(N, L.LD_CRITIC); cobs[:, :475] = torch.randn(N, 475, generator=g)
    carry = buffers.CarryBuffers(N, H, 2, "cuda:0")
    carry.actor_hc.copy_(torch.randn(2, 2, N, H, generator=g) * 0.5)
    carry.critic_hc.copy_(torch.randn(2, 2, N, H, generator=g) * 0.5)
    carry.lpf.copy_(torch.randn(N, 20, generator=g) * 0.3)
    hc_a0, lpf0 = carry.actor_hc.cpu().double(), carry.lpf.cpu().double()
    action, logp, value = torch.zeros(N, 20, device="cuda:0"), torch.zeros(N, device="cuda:0"), torch.zeros(N, device="cuda:0")
    ctx.policy_step(params, aobs.cuda(), cobs.cuda(), carry.c, 7, 5, True, action, logp, value)
    ctx.synchronize()
    out_a, _ = ON.net_forward(p, "actor", aobs[:, :65].double(), [[hc_a0[l, 0], hc_a0[l, 1]] for l in range(2)])
    mean, std, lpf1 = ON.actor_head(out_a, aobs.double(), lpf0, jb, cfg)
    if abs(cfg.max_std - 1.0) > 1e-6:
        assert 0.10 <= float((std >= cfg.max_std).double().mean()) <= 0.90
    e_mu = float((action.cpu().double() - mean).abs().max())
    e_lp = float((logp.cpu().double() - ON.gaussian_logp(mean, mean, std)).abs().max())
    e_lpf = float((carry.lpf.cpu().double() - lpf1).abs().max())
    e_ls = float((-(logp.cpu().double() + 10 * ON.LOG_2PI) - std.log().sum(-1)).abs().max())
    print("hparams policy step %-14s H%d-N%d: mode %.2e logp %.2e lpf %.2e sum log std %.2e" % (name, H, N, e_mu, e_lp, e_lpf, e_ls))
    assert e_mu < 2e-5 and e_lp < 1e-4 and e_lpf < 1e-5 and e_ls < 1e-4
    # a sampled step from the same state: the log-prob is the oracle's density of the sample, the draws are unit Gaussians under the oracle's std
    c2 = buffers.CarryBuffers(N, H, 2, "cuda:0")
    c2.actor_hc.copy_(hc_a0.float()); c2.critic_hc.copy_(carry.critic_hc); c2.lpf.copy_(lpf0.float())
    a1, lp1 = torch.zeros_like(action), torch.zeros_like(logp)
    ctx.policy_step(params, aobs.cuda(), cobs.cuda(), c2.c, 7, 5, False, a1, lp1, value)
    ctx.synchronize()
    assert (lp1.cpu().double() - ON.gaussian_logp(a1.cpu().double(), mean, std)).abs().max() < 1e-3
    z = ((a1.cpu().double() - mean) / std).flatten()
    assert abs(z.mean()) < 0.1 and abs(z.std() - 1) < 0.1
    assert (c2.lpf.cpu().double() - lpf1).abs().max() < 1e-5
    ctx.close()


# ---- 2. AdamW: one step from an arbitrary state ---------------------------------------------------------------------------------------
def _adam_state(torch, P, gscale, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = (torch.rand(P, generator=g) * 2 - 1) * 0.1
    grad = torch.randn(P, generator=g) * gscale
    mom = torch.randn(P, generator=g) * gscale * 0.5
    var = (0.1 + torch.rand(P, generator=g)) * gscale * gscale      # >= 0 and off zero: m / sqrt(v) stays O(1)
    return p, mom, var, grad


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


def _adam_oracles(ON, cfg, p, mom, var, grad, step, gs):
    """One ON.adamw_step from the float32 state in fp64 and in fp32: ((p, m, v) fp64, bounds (p, m, v)). Bound = 4x the fp32 oracle's own max
    error against fp64, not less than one fp32 ulp of the array's largest entry."""
    o64 = [x.double().clone() for x in (p, mom, var)]
    ON.adamw_step(cfg, *o64, grad.double(), step, gs)
    o32 = [x.clone() for x in (p, mom, var)]
    ON.adamw_step(cfg, *o32, grad.clone(), step, gs)
    bounds = [max(4 * float((a.double() - b).abs().max()), _ulp32(float(b.abs().max()))) for a, b in zip(o32, o64)]
    return o64, bounds


# name -> (config overrides, step, grad_scale, gradient magnitude, the same config with the case's term switched off or None)
ADAM_CASES = {
    "defaults-step1": ({}, 1, 1.0, 1e-2, None),
    "weight_decay=0.1,lr=1e-2": (dict(weight_decay=0.1, learning_rate=1e-2), 3, 1.0, 1e-2, dict(weight_decay=0.0, learning_rate=1e-2)),
    "clip-off": (dict(max_grad_norm=1e9), 3, 1.0, 1e-2, None),
    "clip-on": (dict(max_grad_norm=0.01), 3, 0.25, 1e-2, dict(max_grad_norm=1e9)),
    "adam_eps=1e-3": (dict(adam_eps=1e-3), 1000, 1.0, 1e-3, dict(adam_eps=1e-8)),      # sqrt(v_hat) ~ 1e-3 = eps
    "betas=0.5,0.9": (dict(adam_b1=0.5, adam_b2=0.9), 3, 1.0, 1e-2, None),
    "step=1000": ({}, 1000, 1.0, 1e-2, None),
    "step=1e6": ({}, 10 ** 6, 1.0, 1e-2, None),
    "step=2^31+5": ({}, 2 ** 31 + 5, 1.0, 1e-2, None),
}


@pytest.mark.parametrize("H", [64, 100])       # 100: zero padded to 128 inside the library, the step runs on the caller's layout
@pytest.mark.parametrize("name", list(ADAM_CASES))
def test_adamw_step_matches_oracle(name, H):
    """One kbj_adamw_step from a random state (p uniform +-0.1, random gradient / m / v >= 0, `step` given) against ON.adamw_step in fp64, on
    the context's own param_count(). Bounds from the reference at run time (_adam_oracles): the fp32 oracle's own error is ~4e-9 on p and
    ~1e-7 relative on m / v, so p is held to ~1.6e-8 where the smallest intended movement is 9e-5. Where a case exists to pin one term
    (decay, clip, eps), the bound on p must stay <= 1/100 of what that term moves p by on the oracle.
    Measured on an MI355X (worst over the cases): p 4.8e-9 (bound 1.9e-8; 3.8e-9 against 1.5e-8 at the default rate), m 1.8e-9 (7.1e-9),
    v 1.4e-11 (3.9e-11): the device sits at the fp32 oracle's own error, a quarter of each bound."""
    ov, step, gs, gmag, off = ADAM_CASES[name]
    m_, cfg, ctx, torch, buffers = _setup(40, 32, 4, H, **ov)
    from oracle import nn as ON
    P = ctx.param_count()
    assert P == ON.param_count(H) and P % 64 != 0                               # a ragged last wavefront
    p, mom, var, grad = _adam_state(torch, P, gmag, seed=H)
    (p_o, m_o, v_o), (bp, bm, bv) = _adam_oracles(ON, cfg, p, mom, var, grad, step, gs)
    norm = float((grad.double() * gs).norm())
    if "max_grad_norm" in ov:
        assert (norm > 10 * cfg.max_grad_norm) if name == "clip-on" else (norm < 0.1 * cfg.max_grad_norm)     # the clip is certainly on / off
    if off is not None:     # what the pinned term moves p by, on the oracle: the bound must resolve 1/100 of it
        cfg_off = L.default_config(num_envs=40, batch_size=32, rollout_len=4, hidden_size=H, **off)
        p_off = p.double().clone()
        ON.adamw_step(cfg_off, p_off, mom.double().clone(), var.double().clone(), grad.double(), step, gs)
        term = float((p_off - p_o).abs().max())
        assert bp <= term / 100, (name, bp, term)
    assert float((p_o - p.double()).abs().max()) > 100 * bp                      # the step itself is far above the bound
    pd, md, vd, gd = p.cuda(), mom.cuda(), var.cuda(), grad.cuda()
    ctx.adamw_step(pd, md, vd, gd, step, gs)
    ctx.synchronize()
    ep, em, ev = (float((a.cpu().double() - b).abs().max()) for a, b in ((pd, p_o), (md, m_o), (vd, v_o)))
    print("hparams adamw %-26s H%d: p %.2e (bound %.2e) m %.2e (%.2e) v %.2e (%.2e)" % (name, H, ep, bp, em, bm, ev, bv))
    assert ep <= bp and em <= bm and ev <= bv, (name, (ep, bp), (em, bm), (ev, bv))
    assert torch.equal(gd.cpu(), grad)                                           # the gradient is an input
    ctx.close()


@pytest.mark.parametrize("H", [64, 100])
def test_adamw_learning_rate_changes_between_steps(H):
    """kbj_set_learning_rate between steps: a new positive rate, 0 (parameters stay bit-identical, the moments advance) and the documented
    negative rate (the reference's scale_by_schedule chain without a sign flip); the oracle follows with the same rate in its config.
    Bounds as test_adamw_step_matches_oracle, from the fp32 oracle run on the same chain."""
    m_, cfg, ctx, torch, buffers = _setup(40, 32, 4, H)
    from oracle import nn as ON
    P = ctx.param_count()
    p, mom, var, _ = _adam_state(torch, P, 1e-2, seed=7)
    pd, md, vd = p.cuda(), mom.cuda(), var.cuda()
    o64, o32 = [x.double().clone() for x in (p, mom, var)], [x.clone() for x in (p, mom, var)]
    g = torch.Generator(device="cpu").manual_seed(8)
    for step, lr in ((1, None), (2, 2e-3), (3, 0.0), (4, -1e-3)):
        if lr is not None:
            ctx.set_learning_rate(lr)
            cfg = L.default_config(num_envs=40, batch_size=32, rollout_len=4, hidden_size=H, learning_rate=lr)
        grad = torch.randn(P, generator=g) * 1e-2
        before = pd.clone()
        p_before = o64[0].clone()
        ctx.adamw_step(pd, md, vd, grad.cuda(), step, 1.0)
        ctx.synchronize()
        ON.adamw_step(cfg, *o64, grad.double(), step, 1.0)
        ON.adamw_step(cfg, *o32, grad.clone(), step, 1.0)
        bounds = [max(4 * float((a.double() - b).abs().max()), _ulp32(float(b.abs().max()))) for a, b in zip(o32, o64)]
        errs = [float((a.cpu().double() - b).abs().max()) for a, b in zip((pd, md, vd), o64)]
        print("hparams adamw lr %s step %d H%d: p %.2e (bound %.2e) m %.2e v %.2e" % (lr, step, H, errs[0], bounds[0], errs[1], errs[2]))
        assert all(e <= b for e, b in zip(errs, bounds)), (step, lr, errs, bounds)
        if lr == 0.0:
            assert torch.equal(pd, before)
        else:
            moved = o64[0] - p_before
            assert float(moved.abs().max()) > 100 * bounds[0]
            if lr is not None and lr < 0:     # the negative rate steps the other way: along +m_hat on almost every element
                mh = o64[1]
                assert float(((moved * mh) > 0).double().mean()) > 0.99
    ctx.close()


@pytest.mark.parametrize("H", [64, 100])
def test_adamw_chain_of_50_steps_matches_oracle(H):
    """50 steps with a fresh random gradient each (bias corrections 1 .. 50, moments building up from zero): compared after every step with the
    bound the fp32 oracle's own chain gives at that step.
    Measured on an MI355X after 50 steps: p 6.4e-8 (bound 2.6e-7) at H 64, 7.3e-8 (2.9e-7) at H 100."""
    m_, cfg, ctx, torch, buffers = _setup(40, 32, 4, H)
    from oracle import nn as ON
    P = ctx.param_count()
    g = torch.Generator(device="cpu").manual_seed(21)
    p = (torch.rand(P, generator=g) * 2 - 1) * 0.1
    pd, md, vd = p.cuda(), torch.zeros(P, device="cuda:0"), torch.zeros(P, device="cuda:0")
    o64 = [p.double().clone(), torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)]
    o32 = [p.clone(), torch.zeros(P), torch.zeros(P)]
    for step in range(1, 51):
        grad = torch.randn(P, generator=g) * 1e-2
        ctx.adamw_step(pd, md, vd, grad.cuda(), step, 1.0)
        ctx.synchronize()
        ON.adamw_step(cfg, *o64, grad.double(), step, 1.0)
        ON.adamw_step(cfg, *o32, grad.clone(), step, 1.0)
        bounds = [max(4 * float((a.double() - b).abs().max()), _ulp32(float(b.abs().max()))) for a, b in zip(o32, o64)]
        errs = [float((a.cpu().double() - b).abs().max()) for a, b in zip((pd, md, vd), o64)]
        assert all(e <= b for e, b in zip(errs, bounds)), (step, errs, bounds)
    print("hparams adamw chain H%d after 50 steps: p %.2e (bound %.2e) m %.2e (%.2e) v %.2e (%.2e)" % (H, errs[0], bounds[0], errs[1], bounds[1], errs[2], bounds[2]))
    assert float((o64[0] - p.double()).abs().max()) > 5e-3                        # 50 steps of ~lr each
    ctx.close()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_adamw_non_finite_gradient_is_fail_stop(bad):
    """A gradient holding one +inf / one NaN: the step is skipped (parameters and both moments bit-identical), kbj_synchronize reports it, and
    the context serves a following finite step, which matches the oracle. A return-code path of adamw_kernel (err[1]), no device fault."""
    H = 100
    m_, cfg, ctx, torch, buffers = _setup(40, 32, 4, H)
    from kbot_joystick_amd.host.binding import KbjError
    from oracle import nn as ON
    P = ctx.param_count()
    p, mom, var, grad = _adam_state(torch, P, 1e-2, seed=13)
    pd, md, vd = p.cuda(), mom.cuda(), var.cuda()
    poisoned = grad.clone()
    poisoned[P // 3] = bad
    ctx.adamw_step(pd, md, vd, poisoned.cuda(), 5, 1.0)
    with pytest.raises(KbjError, match="non-finite gradient"):
        ctx.synchronize()
    assert torch.equal(pd.cpu(), p) and torch.equal(md.cpu(), mom) and torch.equal(vd.cpu(), var)
    (p_o, m_o, v_o), (bp, bm, bv) = _adam_oracles(ON, cfg, p, mom, var, grad, 5, 1.0)
    ctx.adamw_step(pd, md, vd, grad.cuda(), 5, 1.0)
    ctx.synchronize()                                                            # the flag was acknowledged: no error now
    ep, em, ev = (float((a.cpu().double() - b).abs().max()) for a, b in ((pd, p_o), (md, m_o), (vd, v_o)))
    assert ep <= bp and em <= bm and ev <= bv, ((ep, bp), (em, bm), (ev, bv))
    ctx.close()


# ---- 3. GAE on its own --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma,lam", [(0.94, 0.94), (0.0, 0.94), (0.999, 0.0), (1.0, 1.0)])
def test_gae_matches_oracle(gamma, lam):
    """kbj_gae on synthetic value / reward / done arrays against ON.gae in fp64: N in {1, 63, 257, 1000} (one lane, ragged wavefronts), T in
    {1, 2, 100} (the bootstrap V_T := V_{T-1} alone, once, and a long scan), done patterns none / all / last step only / random 15 % of both
    signs. Bound 1e-5 (1 + |reference|): the fp32 oracle itself stays within 5e-7 of that form, including (1, 1) where |adv| reaches 58.
    Measured on an MI355X (worst over all shapes and patterns, in units of 1 + |reference|): 6.4e-7, |adv| up to 59.9
    at (1, 1)."""
    m_, cfg, ctx, torch, buffers = _setup(40, 32, 4, 64, gamma=gamma, lam=lam)
    from kbot_joystick_amd.host import binding as Bd
    from oracle import nn as ON
    g = torch.Generator(device="cpu").manual_seed(17)
    worst, reach = 0.0, 0.0
    for N in (1, 63, 257, 1000):
        for T in (1, 2, 100):
            value, reward = torch.randn(T, N, generator=g), torch.rand(T, N, generator=g)
            rnd = (torch.rand(T, N, generator=g) < 0.15).float() * torch.where(torch.rand(T, N, generator=g) < 0.5, -1.0, 1.0)
            last = torch.zeros(T, N); last[T - 1] = 1.0
            for pattern, done in (("none", torch.zeros(T, N)), ("all", torch.ones(T, N)), ("last", last), ("random", rnd)):
                aux = torch.zeros(T, N, L.AUX["SIZE"])
                aux[:, :, L.AUX["DONE"]] = done
                aux_d, value_d, reward_d = aux.cuda(), value.cuda(), reward.cuda()
                adv_d, tgt_d = torch.full((T, N), 7.0, device="cuda:0"), torch.full((T, N), 7.0, device="cuda:0")
                tr = Bd.Traj(T, N, None, None, aux_d.data_ptr(), None, None, value_d.data_ptr(), reward_d.data_ptr(), None, None, None, None, None, None, None, None)
                ctx.gae(tr, adv_d, tgt_d)
                ctx.synchronize()
                adv_o, tgt_o = ON.gae(value.double(), reward.double(), done.double(), cfg.gamma, cfg.lam)
                for got, ref in ((adv_d, adv_o), (tgt_d, tgt_o)):
                    e = float(((got.cpu().double() - ref).abs() / (1 + ref.abs())).max())
                    worst = max(worst, e)
                    assert e < 1e-5, (N, T, pattern, e)
                reach = max(reach, float(adv_o.abs().max()))
    print("hparams gae gamma %.3f lam %.3f: worst %.2e (1 + |ref|), |adv| up to %.1f" % (gamma, lam, worst, reach))
    ctx.close()
