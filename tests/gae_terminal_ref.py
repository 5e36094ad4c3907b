"""The gae_terminal_value row of kbj_gae's table (include/kbj.h) in float64 numpy: tests/gae_ref.py's scan with one case changed - at a truncation
(DONE > 0) the bootstrap is value_term[t][n], the critic's value of the observation the episode ended in, instead of V(s_t). Shared by
tests/test_terminal_value_host.py and tests/test_gpu_terminal_value.py."""
import numpy as np

from tests import gae_ref as G


def gae_terminal_ref(value, reward, done, gamma, lam, value_term, tail=None):
    """value / reward / done / value_term [T, N]; tail [N] = V(s_T) (gae_tail_value = 1) or None. gae_bootstrap_truncation = 1 is implied
    (kbj_check_config refuses the new switch without it). Returns (adv, target) [T, N] float64."""
    value, reward, done, value_term = (np.asarray(x, np.float64) for x in (value, reward, done, value_term))
    gamma, lam = float(gamma), float(lam)
    T, N = value.shape
    adv = np.zeros((T, N), np.float64)
    for n in range(N):
        a_next = 0.0
        for t in range(T - 1, -1, -1):
            d, v, r = done[t, n], value[t, n], reward[t, n]
            if d < 0:
                a = r - v                                       # terminal: nothing follows
            elif d > 0:
                a = r + gamma * value_term[t, n] - v            # truncation: the terminal observation's value; still cut (the last row too)
            elif t < T - 1:
                a = r + gamma * value[t + 1, n] - v + gamma * lam * a_next
            else:
                vn = v if tail is None else float(tail[n])
                a = r + gamma * vn - v
            adv[t, n] = a_next = a
    return adv, adv + value


def gae_terminal_bound(value, reward, tail, value_term, adv_ref, gamma, lam):
    """tests/gae_ref.gae_bound with the terminal values among the bootstrap operands: the derivation bounds every bootstrapped quantity by the
    largest |value| it can be, and value_term[t][n] now is one of them (it takes V(s_t)'s place in the same six roundings)."""
    boot = np.abs(np.asarray(value_term, np.float64)).ravel()
    if tail is not None:
        boot = np.concatenate([boot, np.abs(np.asarray(tail, np.float64)).ravel()])
    return G.gae_bound(value, reward, boot, adv_ref, gamma, lam)


def affected_rows(done):
    """[T, N] bool: the rows a change of the terminal values can reach - every truncation row (DONE > 0) and the rows in front of it in the same
    env up to, not including, the previous row with DONE != 0 (their advantages chain into the truncation row's; behind it the chain is cut)."""
    done = np.asarray(done)
    T, N = done.shape
    out = np.zeros((T, N), bool)
    for n in range(N):
        live = False
        for t in range(T - 1, -1, -1):
            if done[t, n] > 0:
                live = True
            elif done[t, n] < 0:
                live = False
            out[t, n] = live
    return out
