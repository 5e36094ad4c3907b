"""Host restatement of kbj_gae with its selectable boundary conventions (include/kbj.h; kbj_config.gae_bootstrap_truncation / gae_tail_value):
the table of the header, case by case, in float64 numpy. Shared by tests/test_gae_boundary_host.py and tests/test_gpu_gae_boundary.py."""
import numpy as np


def gae_ref(value, reward, done, gamma, lam, bootstrap_truncation=0, tail=None):
    """value / reward / done [T, N]; tail [N] = V(s_T) (gae_tail_value = 1) or None (= 0: V_T := V_{T-1}). Returns (adv, target) [T, N] float64."""
    value, reward, done = (np.asarray(x, np.float64) for x in (value, reward, done))
    gamma, lam = float(gamma), float(lam)
    T, N = value.shape
    adv = np.zeros((T, N), np.float64)
    for n in range(N):
        a_next = 0.0
        for t in range(T - 1, -1, -1):
            d, v, r = done[t, n], value[t, n], reward[t, n]
            if d < 0 or (d > 0 and not bootstrap_truncation):
                a = r - v                                       # terminal: nothing follows
            elif d > 0:
                a = r + gamma * v - v                           # truncation: V(s_t) stands in for the unrecorded terminal observation; still cut
            elif t < T - 1:
                a = r + gamma * value[t + 1, n] - v + gamma * lam * a_next
            else:
                vn = v if tail is None else float(tail[n])
                a = r + gamma * vn - v
            adv[t, n] = a_next = a
    return adv, adv + value


def gae_bound(value, reward, tail, adv_ref, gamma, lam):
    """The rounding bound of the fp32 kernel against gae_ref: a step does at most six fp32 roundings of quantities bounded by
    S = max|r| + (1 + gamma) max(|v|, |tail|) + gamma lam max|A_ref|, and the error decays with gamma lam:
    6 * 2^-24 * S * min(T, 1 / (1 - gamma lam)) (T when gamma lam = 1)."""
    gamma, lam = float(gamma), float(lam)
    T = np.asarray(value).shape[0]
    vmax = float(np.abs(value).max())
    if tail is not None:
        vmax = max(vmax, float(np.abs(tail).max()))
    S = float(np.abs(reward).max()) + (1.0 + gamma) * vmax + gamma * lam * float(np.abs(adv_ref).max())
    gl = gamma * lam
    return 6.0 * 2.0 ** -24 * S * (T if gl >= 1.0 else min(T, 1.0 / (1.0 - gl)))


def boundary_problem(N, T, seed=0):
    """The synthetic trajectory of the PPO parity tests (helpers.synthetic_arrays(N, T, 64, 0): rewards in [0, 1), 15 % of the steps done, half of
    them +1) with `value` [T, N] and `tail` [N] drawn as standard normals from a fixed generator: float32 numpy arrays by name."""
    import torch
    from tests import helpers
    arr = helpers.synthetic_arrays(N, T, 64, 0)
    g = torch.Generator(device="cpu").manual_seed(1234 + seed)
    return dict(done=arr["done"].numpy(), reward=arr["reward"].numpy(), value=torch.randn(T, N, generator=g).numpy(), tail=torch.randn(N, generator=g).numpy())
