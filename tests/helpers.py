"""Shared helpers for the parity tests: env side first, the actor-critic / PPO side (synthetic minibatch problems against oracle/nn.py) below."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Parity tolerances for ONE control step (5 substeps) started from the identical fp32 state, MEASURED (profiles/parity_r02.json,
# tools/parity_quantiles.py: 8192 envs x 12 teacher-forced steps, errors against the fp64 oracle):
#              median     p99      p99.9    max
#   HIP  qpos  1.8e-7   7.8e-7   1.4e-6   4.2e-2      oracle fp32  qpos  1.8e-7   8.6e-7   1.6e-6   4.2e-2
#   HIP  qvel  6.6e-7   3.8e-6   7.5e-6   5.4e-1      oracle fp32  qvel  7.2e-7   4.3e-6   8.3e-6   3.3e-1
#   HIP  qacc  2.6e-6   1.7e-5   3.9e-5   1.7e+0      oracle fp32  qacc  2.9e-6   2.0e-5   4.7e-5   4.6e-1
# i.e. the kernel is as close to fp64 as the oracle's own fp32 instantiation, at every quantile. The table below is 2x the oracle's
# own fp32 spread for (median, p99, p99.9); the tests that have the fp64 oracle at hand (check_against_oracle_spread) compare with
# the spread measured in the same run instead of with these constants. The extreme value is set by a handful of env-steps that sit
# on a discrete switch of the solver (contact on/off, friction row saturating, Newton iteration cap: 0.02 % of env-steps, the same
# share in the oracle's fp32-vs-fp64 comparison) and is bounded relative to the oracle's own extreme value.
TOL = dict(qpos=(4e-7, 2e-6, 4e-6, 0.1), qvel=(1.5e-6, 1e-5, 2e-5, 1.0), qacc=(6e-6, 4e-5, 1e-4, 4.0))   # (median, p99, p99.9, max)


def emu_lib(solver: str = "reg", sanitize: bool = False) -> C.CDLL:
    """Host emulation build of the kernel body (tests/emu) — test infrastructure. solver = "reg": the product kernel's register-resident
    Newton solver, its wave primitives (DPP broadcasts, butterflies, lane swaps) emulated lane by lane (kbj_wave.h); "lds": the LDS
    formulation that `make ldssolver` builds for the GPU A/B test. sanitize: -fsanitize=address,undefined (load it in a child process
    with libasan preloaded, tests/test_sanitize.py)."""
    name = "libkbj_emu" + ("" if solver == "reg" else "_lds") + ("_asan" if sanitize else "") + ".so"
    out = os.path.join(ROOT, "tests", "emu", "_build", name)
    src = os.path.join(ROOT, "tests", "emu", "kbj_env_emu.cpp")
    deps = [src] + [os.path.join(ROOT, "kbot-joystick_amd", "csrc", f) for f in ("kbj_env_core.h", "kbj_env_phys.h", "kbj_env_task.h", "kbj_wave.h")]
    deps.append(os.path.join(ROOT, "include", "kbj_model.h"))
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
        if solver == "lds":
            flags.append("-DKBJ_ARROW_LDS")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                               "-shared", "-o", out, src])
    return C.CDLL(out) if not sanitize else out


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def state_errors(es_ref: np.ndarray, es_got: np.ndarray):
    """Per-env error measures between two [N][ES] state arrays."""
    d = np.abs(es_ref.astype(np.float64) - es_got.astype(np.float64))
    return dict(qpos=d[:, 0:27].max(1),
                qvel=d[:, 28:54].max(1) / (1 + np.abs(es_ref[:, 28:54]).max(1)),
                qacc=d[:, 54:80].max(1) / (1 + np.abs(es_ref[:, 54:80]).max(1)))


def check_error_distribution(errs: dict, tol=TOL, label=""):
    for k, (med, p99, p999, mx) in tol.items():
        v = np.concatenate(errs[k])
        assert np.median(v) <= med, f"{label}{k}: median {np.median(v):.3e} > {med}"
        assert np.quantile(v, 0.99) <= p99, f"{label}{k}: p99 {np.quantile(v, 0.99):.3e} > {p99}"
        if v.size >= 20000:     # a 99.9th percentile needs samples
            assert np.quantile(v, 0.999) <= p999, f"{label}{k}: p99.9 {np.quantile(v, 0.999):.3e} > {p999}"
        assert v.max() <= mx, f"{label}{k}: max {v.max():.3e} > {mx}"


def check_against_oracle_spread(err_hip: dict, err_o32: dict, switch: np.ndarray, label=""):
    """HIP-vs-fp64 error distribution against the oracle's own fp32-vs-fp64 distribution measured on the SAME env-steps:
      * median, p99, p99.9 at most 2x the oracle's (floored at a few fp32 roundings of the quantity);
      * no heavier tail: the count of env-steps beyond 2x the oracle's p99.9 is at most 1.5x the oracle's own count (+5);
      * the extreme value inside the absolute bound of the tolerance table (a single env-step on a discrete switch sets it, in
        the oracle's fp32-vs-fp64 comparison just the same: the ratio of two such extremes is not a stable statistic);
      * beyond 2x the oracle's p99.9, at most 8 env-steps that the oracle does not itself flag as sitting on a discrete switch of
        the solver (`switch`: active contacts / force-carrying rows / iteration counts differ between two evaluations that differ
        only by rounding, or the iteration cap bites) - measured: 2-3 of 98k, the kernel's own rounding flips a switch there."""
    floor = dict(qpos=2e-7, qvel=1e-6, qacc=4e-6)
    sw = np.concatenate(switch)
    for k in ("qpos", "qvel", "qacc"):
        h, o = np.concatenate(err_hip[k]), np.concatenate(err_o32[k])
        for name, q in (("median", 0.5), ("p99", 0.99), ("p99.9", 0.999)):
            hq, oq = np.quantile(h, q), np.quantile(o, q)
            assert hq <= 2 * max(oq, floor[k]), f"{label}{k} {name}: HIP {hq:.3e} vs oracle fp32 {oq:.3e}"
        thr = 2 * np.quantile(o, 0.999)
        nh, no = int((h > thr).sum()), int((o > thr).sum())
        assert nh <= 1.5 * no + 5, f"{label}{k}: {nh} env-steps beyond {thr:.2e}, the oracle's fp32 run has {no}"
        assert h.max() <= TOL[k][3], f"{label}{k}: max {h.max():.3e} (oracle fp32 max {o.max():.3e})"
        unexplained = int(((h > thr) & ~sw).sum())
        assert unexplained <= 8, f"{label}{k}: {unexplained} outliers beyond {thr:.2e} on env-steps without a discrete solver switch"


def random_actions(model, rng, n, scale=0.3):
    return (np.tile(np.array(model.joint_bias, np.float32), (n, 1)) + rng.normal(size=(n, 20)).astype(np.float32) * scale)


# ---------------------------------------------------------------------------------------------------------------------
# actor-critic / PPO side: the synthetic minibatch problem of tests/test_gpu_nn.py as CPU tensors, so that the oracle half of a
# parity test (and the CPU-only liveness checks of tests/test_oracle_nn.py) needs no device
# ---------------------------------------------------------------------------------------------------------------------
# The update's hyperparameters at non-default values (tests/test_gpu_hparams.py; liveness on the oracle alone in tests/test_oracle_nn.py).
# name -> kbj_config overrides. Each case must move the oracle's gradient by >= 1e-2 of its norm (100x the parity bound): measured on
# the CPU at both shapes below, the smallest is 3.2e-2 (value_clip 0.05); the table is in tests/test_oracle_nn.py.
HPARAM_CASES = {
    "entropy_coef=0.5": dict(entropy_coef=0.5),
    "value_loss_coef=2": dict(value_loss_coef=2.0),
    "clip_param=0.05": dict(clip_param=0.05),
    "clip_param=0.6": dict(clip_param=0.6),
    "value_clip=0.05": dict(value_clip=0.05),
    "value_clip=5": dict(value_clip=5.0),
    "log_ratio_clip=0.25": dict(log_ratio_clip=0.25),
    "adv_eps=0.5": dict(adv_eps=0.5),
    "max_std=0.35": dict(max_std=0.35),
    "min_std=0.2": dict(min_std=0.2),
    "var_scale=1.5": dict(var_scale=1.5),       # pushes 78 % / 97 % of the std elements into the default max_std = 1 clamp ...
    "var_scale=0.25": dict(var_scale=0.25),     # ... so a second value that stays below it: the scale's own gradient factor on every element
    "lpf_alpha=1": dict(lpf_alpha=1.0),
    "lpf_alpha=0.1": dict(lpf_alpha=0.1),
    "gamma=0": dict(gamma=0.0),
    "gamma=1,lam=1": dict(gamma=1.0, lam=1.0),
    "lam=0": dict(lam=0.0),
    "combined": dict(entropy_coef=0.1, value_loss_coef=1.5, clip_param=0.1, value_clip=0.1, log_ratio_clip=0.4, adv_eps=0.1, max_std=0.6,
                     min_std=0.05, var_scale=0.8, lpf_alpha=0.3, gamma=0.9, lam=0.8),
}
HPARAM_HEAD_CASES = ["max_std=0.35", "min_std=0.2", "var_scale=1.5", "var_scale=0.25", "lpf_alpha=1", "lpf_alpha=0.1"]     # the fields the forward-only passes read
# (H, N, B, T): one small and ragged; one at H = 256 whose 12 steps cross the 10-step fetch chunks of the head's time scans
HPARAM_SHAPES = [(64, 40, 32, 9), (256, 40, 32, 12)]


def init_like_params(H, seed, depth=2):
    """A CPU draw from the distribution of kbj_init_params (uniform +-1/sqrt(fan_in) per leaf; not its stream): fp64 flat vector."""
    import torch
    from oracle import nn as ON
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for name, shp in ON.param_shapes(H, depth):
        fan_in = shp[1] if name.endswith("input_proj.weight") else (ON.NOBS_ACTOR if name == "actor.input_proj.bias" else ON.NOBS_CRITIC if name == "critic.input_proj.bias" else H)
        out.append((torch.rand(int(np.prod(shp)), generator=g, dtype=torch.float64) * 2 - 1) / np.sqrt(fan_in))
    return torch.cat(out)


def synthetic_arrays(N, T, H, seed=0, depth=2, mirror=False):
    """The synthetic trajectory of the PPO parity tests as CPU float32 tensors (rows padded as the device rows are): name -> tensor."""
    import torch
    from kbot_joystick_amd.spec import layout as L
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = dict(actor_obs=torch.zeros(T + 1, N, L.LD_ACTOR), critic_obs=torch.zeros(T + 1, N, L.LD_CRITIC))
    a["actor_obs"][:, :, :65] = torch.randn(T + 1, N, 65, generator=g) * 0.5
    a["critic_obs"][:, :, :475] = torch.randn(T + 1, N, 475, generator=g) * 0.5
    a["action"] = torch.randn(T, N, 20, generator=g) * 0.3
    a["done"] = (torch.rand(T, N, generator=g) < 0.15).float() * torch.where(torch.rand(T, N, generator=g) < 0.5, -1.0, 1.0)
    a["reward"] = torch.rand(T, N, generator=g)
    a["carry0_actor_hc"] = torch.randn(depth, 2, N, H, generator=g) * 0.3
    a["carry0_critic_hc"] = torch.randn(depth, 2, N, H, generator=g) * 0.3
    a["carry0_lpf"] = torch.randn(N, 20, generator=g) * 0.2
    if mirror:
        a["carry0_actor_mirror_hc"] = torch.randn(depth, 2, N, H, generator=g) * 0.3
        a["carry0_critic_mirror_hc"] = torch.randn(depth, 2, N, H, generator=g) * 0.3
        a["carry0_lpf_mirror"] = torch.randn(N, 20, generator=g) * 0.2
    return a


def fill_traj(tr, arr):
    """Copy synthetic_arrays() into a TrajBuffers of the same shape."""
    from kbot_joystick_amd.spec import layout as L
    T = tr.T
    tr.actor_obs.copy_(arr["actor_obs"]); tr.critic_obs.copy_(arr["critic_obs"])
    tr.action.copy_(arr["action"])
    tr.aux[:T, :, L.AUX["DONE"]] = arr["done"].to(tr.aux.device)
    tr.reward.copy_(arr["reward"])
    for k in ("carry0_actor_hc", "carry0_critic_hc", "carry0_lpf", "carry0_actor_mirror_hc", "carry0_critic_mirror_hc", "carry0_lpf_mirror"):
        if k in arr:
            getattr(tr, k).copy_(arr[k])
    for k in ("logp", "value"):
        if k in arr:
            getattr(tr, k).copy_(arr[k])


def _carry(arr, key, ii, depth):
    c = arr[key].double()
    return [[c[l, k] if ii is None else c[l, k][ii] for k in range(2)] for l in range(depth)]


def oracle_head_series(p, cfg, jb, arr, ii=None, depth=2):
    """The actor head over the trajectory on the oracle (no gradient): (filtered mean [T,B,20], std [T,B,20]) for the envs `ii` (None: all)."""
    import torch
    from oracle import nn as ON
    T = arr["action"].shape[0]
    sel = (lambda x: x) if ii is None else (lambda x: x[:, ii])
    ao, done = sel(arr["actor_obs"][:T].double()), sel(arr["done"].double())
    ca, lpf = _carry(arr, "carry0_actor_hc", ii, depth), (arr["carry0_lpf"].double() if ii is None else arr["carry0_lpf"].double()[ii])
    means, stds = [], []
    with torch.no_grad():
        for t in range(T):
            out_a, ca = ON.net_forward(p, "actor", ao[t], ca, depth)
            mean, std, lpf = ON.actor_head(out_a, ao[t], lpf, jb, cfg)
            means.append(mean); stds.append(std)
            keep = (done[t] == 0).double()[:, None]
            ca = [[h * keep, c * keep] for h, c in ca]
            lpf = lpf * keep
    return torch.stack(means), torch.stack(stds)


def oracle_old_policy(cfg, jb, p64, arr, H, g, depth=2):
    """Old log-probs / values of the synthetic problem: the oracle's own under `cfg` plus N(0, 0.3) noise drawn from `g` (so that some
    ratios leave the clip range), rounded to the float32 the device arrays hold. Returns (logp_old, value_old, (lp, v, en) noise-free)."""
    import torch
    from oracle import nn as ON
    T, N = arr["action"].shape[:2]
    with torch.no_grad():
        lp, v, en, *_ = ON.ppo_variables(ON.unflatten(p64, H, depth), cfg, jb, arr["actor_obs"][:T].double(), arr["critic_obs"][:T].double(), arr["action"].double(),
                                         arr["done"].double(), _carry(arr, "carry0_actor_hc", None, depth), _carry(arr, "carry0_critic_hc", None, depth),
                                         arr["carry0_lpf"].double(), depth)
    logp_old = (lp + 0.3 * torch.randn(T, N, generator=g).double()).float()
    value_old = (v + 0.3 * torch.randn(T, N, generator=g).double()).float()
    return logp_old, value_old, (lp, v, en)


def oracle_minibatch_grad(cfg, jb, p64, arr, idx, H, adv, target, adv_sums=None, depth=2, dtype=None):
    """Autograd of ON.ppo_loss(ON.ppo_variables(...)) over the minibatch `idx` of the synthetic problem; arr["logp"] / arr["value"] are the old
    policy's, adv / target [T, N]. dtype: torch.float32 reruns the same loss in fp32. Returns (flat gradient, metrics dict of floats, logp)."""
    import torch
    from oracle import nn as ON
    dt = dtype or torch.float64
    T = arr["action"].shape[0]
    ii = idx.long()
    pf = p64.to(dt).clone().requires_grad_(True)
    sel = lambda x: x.to(dt)[:, ii]
    cst = lambda c: [[x.to(dt) for x in hc] for hc in c]
    lp, v, en, *_ = ON.ppo_variables(ON.unflatten(pf, H, depth), cfg, jb.to(dt), sel(arr["actor_obs"][:T]), sel(arr["critic_obs"][:T]), sel(arr["action"]), sel(arr["done"]),
                                     cst(_carry(arr, "carry0_actor_hc", ii, depth)), cst(_carry(arr, "carry0_critic_hc", ii, depth)), arr["carry0_lpf"].to(dt)[ii], depth)
    loss, mt = ON.ppo_loss(cfg, lp, v, en, sel(arr["logp"]), sel(arr["value"]), sel(adv), sel(target), adv_sums=adv_sums)
    loss.backward()
    return pf.grad.double(), {k: float(x.detach()) for k, x in mt.items()}, lp.detach().double()


METRIC_NAMES = ["loss", "policy", "value", "entropy", "clipfrac", "kl", "adv_mean", "adv_std"]


def hparam_problem(cfg, jb, p64, arr, H, N, B):
    """The synthetic minibatch problem under `cfg` on the oracle alone: the minibatch indices, the old policy drawn under `cfg`, GAE with
    cfg's gamma / lambda, the fp64 autograd gradient and what the liveness conditions need. Returns a dict; arr gains "logp" / "value"."""
    import torch
    from oracle import nn as ON
    g = torch.Generator(device="cpu").manual_seed(5)
    idx = torch.randperm(N, generator=g)[:B].int()
    arr = dict(arr)
    arr["logp"], arr["value"], _ = oracle_old_policy(cfg, jb, p64, arr, H, g)
    adv, tgt = ON.gae(arr["value"].double(), arr["reward"].double(), arr["done"].double(), cfg.gamma, cfg.lam)
    grad, mt, lp = oracle_minibatch_grad(cfg, jb, p64, arr, idx, H, adv, tgt)
    _, std = oracle_head_series(ON.unflatten(p64, H), cfg, jb, arr, idx.long())
    dlp = (lp - arr["logp"].double()[:, idx.long()]).abs()
    return dict(arr=arr, idx=idx, adv=adv, target=tgt, grad=grad, metrics=mt,
                frac_beyond_lrclip=float((dlp >= cfg.log_ratio_clip).double().mean()), frac_std_clamped=float((std >= cfg.max_std).double().mean()))


def check_hparam_liveness(name, cfg, case, default):
    """The conditions that make a hyperparameter case a test of its term (tests/test_gpu_hparams.py): asserted, not measured."""
    diff = float((case["grad"] - default["grad"]).norm() / case["grad"].norm())
    assert diff >= 1e-2, (name, "the override moves the oracle's gradient by only", diff)
    assert 0.02 < case["metrics"]["clipfrac"] < 0.98, (name, case["metrics"]["clipfrac"])
    if abs(cfg.log_ratio_clip - 10.0) > 1e-6:
        assert case["frac_beyond_lrclip"] >= 0.10, (name, case["frac_beyond_lrclip"])
    if abs(cfg.max_std - 1.0) > 1e-6:
        assert 0.10 <= case["frac_std_clamped"] <= 0.90, (name, case["frac_std_clamped"])
    return diff


def check_grad_parity(gg, go, H, depth=2, label=""):
    """The gradient bounds of tests/test_gpu_nn.py: per leaf max error / leaf max < 2e-3, global relative L2 < 1e-4. Returns the two worst figures."""
    from oracle import nn as ON
    off, worst = 0, 0.0
    for name, shp in ON.param_shapes(H, depth):
        n = int(np.prod(shp))
        a, b = gg[off:off + n], go[off:off + n]
        err = float((a - b).abs().max() / (b.abs().max() + 1e-12))
        worst = max(worst, err)
        assert err < 2e-3, (label, name, err, float(b.abs().max()))
        off += n
    assert off == go.numel()
    rel = float((gg - go).norm() / go.norm())
    assert rel < 1e-4, (label, rel)
    return worst, rel


def check_metrics_parity(mg, mt, label=""):
    """metrics[0..7] of kbj_ppo_grad against the oracle's dict: 2e-4 * (1 + |x|)."""
    worst = 0.0
    for k, name in enumerate(METRIC_NAMES):
        e = abs(float(mg[k]) - mt[name])
        worst = max(worst, e / (1 + abs(mt[name])))
        assert e < 2e-4 * (1 + abs(mt[name])), (label, name, float(mg[k]), mt[name])
    return worst
