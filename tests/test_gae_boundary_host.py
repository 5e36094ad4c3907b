"""The selectable GAE boundary conventions without a device: the float64 restatement (tests/gae_ref.py) against closed forms and against the
oracle's default, the liveness of both switches on the problems the GPU tests use (asserted on the reference alone, so that a kernel which
ignores a switch cannot pass tests/test_gpu_gae_boundary.py), and the plumbing: kbj_check_config, struct mirrors, the two environment
variables, the checkpoint's config member."""
import ctypes
import dataclasses

import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import gae_ref as G

SHAPES = [(40, 9), (70, 12), (130, 100)]       # (N, T); the GPU cases use the first and the last


def _closed(done, bt, tail_on):
    g, l, w = 0.9, 0.7, 1.7
    r, v = np.array([0.3, -0.2, 0.5]), np.array([1.1, -0.6, 0.8])
    adv, tgt = G.gae_ref(v[:, None], r[:, None], np.array(done, np.float64)[:, None], g, l, bt, np.array([w]) if tail_on else None)
    assert np.allclose(tgt, adv + v[:, None], rtol=0, atol=0)
    return adv[:, 0], r, v, g, l, w


def test_closed_form_three_steps():
    """T = 3, one env, done = [0, +1, 0]: every row of the table in include/kbj.h by hand."""
    A, r, v, g, l, w = _closed([0, 1, 0], 1, True)
    A2, A1 = r[2] + g * w - v[2], r[1] + g * v[1] - v[1]
    assert np.allclose(A, [r[0] + g * v[1] - v[0] + g * l * A1, A1, A2], rtol=0, atol=1e-15)
    A, *_ = _closed([0, 1, 0], 0, True)                     # truncation switch off: +1 is terminal
    A1 = r[1] - v[1]
    assert np.allclose(A, [r[0] + g * v[1] - v[0] + g * l * A1, A1, r[2] + g * w - v[2]], rtol=0, atol=1e-15)
    A, *_ = _closed([0, 1, 0], 1, False)                    # tail switch off: V_T := V_{T-1}
    A1 = r[1] + g * v[1] - v[1]
    assert np.allclose(A, [r[0] + g * v[1] - v[0] + g * l * A1, A1, r[2] + g * v[2] - v[2]], rtol=0, atol=1e-15)
    on, off = _closed([0, -1, 0], 1, True)[0], _closed([0, -1, 0], 0, True)[0]
    assert np.array_equal(on, off)                          # a failure is terminal whatever the truncation switch says
    A1 = r[1] - v[1]
    assert np.allclose(on, [r[0] + g * v[1] - v[0] + g * l * A1, A1, r[2] + g * w - v[2]], rtol=0, atol=1e-15)
    # a truncation in the LAST row follows the truncation rule, not the tail rule (row T is a post-reset observation there)
    A, *_ = _closed([0, 0, 1], 1, True)
    assert abs(A[2] - (r[2] + g * v[2] - v[2])) < 1e-15
    A, *_ = _closed([0, 0, 1], 0, True)
    assert abs(A[2] - (r[2] - v[2])) < 1e-15


@pytest.mark.parametrize("N,T", SHAPES)
def test_default_equals_the_oracle(N, T):
    import torch
    from oracle import nn as ON
    p = G.boundary_problem(N, T)
    v, r, d = (torch.from_numpy(p[k]).double() for k in ("value", "reward", "done"))
    for gamma, lam in ((0.94, 0.94), (1.0, 1.0), (0.9, 0.0), (float(np.float32(0.94)), float(np.float32(0.94)))):
        adv, tgt = G.gae_ref(p["value"], p["reward"], p["done"], gamma, lam)
        ao, to = ON.gae(v, r, d, gamma, lam)
        # exact: with keep in {0, 1} the oracle's products and sums are the table's, operation for operation, in float64
        assert np.array_equal(adv, ao.numpy()) and np.array_equal(tgt, to.numpy())


@pytest.mark.parametrize("N,T", SHAPES)
def test_each_switch_moves_the_reference(N, T):
    """Liveness: each switch moves max|adv| by at least 100 x the GPU test's tolerance, and the last row holds every case."""
    p = G.boundary_problem(N, T)
    gamma = lam = float(np.float32(0.94))
    base, _ = G.gae_ref(p["value"], p["reward"], p["done"], gamma, lam)
    trunc, _ = G.gae_ref(p["value"], p["reward"], p["done"], gamma, lam, 1)
    tail, _ = G.gae_ref(p["value"], p["reward"], p["done"], gamma, lam, 0, p["tail"])
    both, _ = G.gae_ref(p["value"], p["reward"], p["done"], gamma, lam, 1, p["tail"])
    tol = max(G.gae_bound(p["value"], p["reward"], p["tail"], a, gamma, lam) for a in (trunc, tail, both))
    assert tol <= 1.2e-3
    d_trunc, d_tail = np.abs(trunc - base).max(), np.abs(tail - base).max()
    print(f"(N, T) = ({N}, {T}): truncation switch moves adv by {d_trunc:.3g}, tail switch by {d_tail:.3g}, tolerance {tol:.3g}; "
          f"truncated {int((p['done'] > 0).sum())}, failed {int((p['done'] < 0).sum())}, last row {int((p['done'][-1] > 0).sum())} / "
          f"{int((p['done'][-1] < 0).sum())} / {int((p['done'][-1] == 0).sum())}")
    assert d_trunc >= 100 * tol and d_tail >= 100 * tol
    assert np.abs(both - trunc).max() >= 100 * tol and np.abs(both - tail).max() >= 100 * tol      # ... and with the other one on
    last = p["done"][-1]
    assert (last > 0).sum() >= 1 and (last < 0).sum() >= 1 and (last == 0).sum() >= 1
    # the switches touch what the table says and nothing else: failures and their predecessors' chains are cut either way
    assert np.array_equal(trunc[p["done"] < 0], base[p["done"] < 0]) and np.array_equal(tail[:, last != 0], base[:, last != 0])


def test_check_config_refuses_other_values():
    from kbot_joystick_amd.host import binding
    ok = lambda **kw: binding.check_config(L.default_config(num_envs=64, batch_size=64, **kw))
    assert ok() == "" and ok(gae_bootstrap_truncation=1) == "" and ok(gae_tail_value=1) == "" and ok(gae_bootstrap_truncation=1, gae_tail_value=1) == ""
    for bad in (2, -1):
        assert "gae_bootstrap_truncation" in ok(gae_bootstrap_truncation=bad)
        assert "gae_tail_value" in ok(gae_tail_value=bad)


def test_struct_mirrors():
    from kbot_joystick_amd.host import binding
    lib = binding.load_library()
    assert lib.kbj_sizeof_config() == ctypes.sizeof(L.Config) and lib.kbj_sizeof_traj() == ctypes.sizeof(binding.Traj)
    c = L.default_config()
    assert (c.gae_bootstrap_truncation, c.gae_tail_value) == (0, 0)
    # the two ints sit between gemm_bf16x3 and dt, the pointer at the end of kbj_traj
    assert L.Config.gae_bootstrap_truncation.offset == L.Config.gemm_bf16x3.offset + 4 and L.Config.dt.offset == L.Config.gae_tail_value.offset + 4
    assert binding.Traj.value_tail_d.offset == binding.Traj.qstate_d.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(binding.Traj) - ctypes.sizeof(ctypes.c_void_p)
    assert "kbj_critic_value" in binding.SIGNATURES and hasattr(lib, "kbj_critic_value")


def test_config_fields_environment_and_checkpoint(tmp_path, monkeypatch):
    from kbot_joystick_amd.host import ckpt
    from kbot_joystick_amd.host.task import HumanoidWalkingTaskConfig, launch_config
    monkeypatch.delenv("KBJ_GAE_TRUNCATION", raising=False); monkeypatch.delenv("KBJ_GAE_TAIL", raising=False)
    c = HumanoidWalkingTaskConfig()
    assert c.bootstrap_on_truncation is False and c.bootstrap_tail_value is False
    k = launch_config().to_kbj(4096)
    assert (k.gae_bootstrap_truncation, k.gae_tail_value) == (0, 0)
    monkeypatch.setenv("KBJ_GAE_TRUNCATION", "1")
    c = launch_config()
    assert c.bootstrap_on_truncation is True and c.bootstrap_tail_value is False
    k = c.to_kbj(4096)
    assert (k.gae_bootstrap_truncation, k.gae_tail_value) == (1, 0)
    monkeypatch.setenv("KBJ_GAE_TRUNCATION", "0"); monkeypatch.setenv("KBJ_GAE_TAIL", "1")
    k = launch_config().to_kbj(4096)
    assert (k.gae_bootstrap_truncation, k.gae_tail_value) == (0, 1)
    monkeypatch.delenv("KBJ_GAE_TRUNCATION"); monkeypatch.delenv("KBJ_GAE_TAIL")
    k = launch_config(bootstrap_on_truncation=True, bootstrap_tail_value=True).to_kbj(4096)      # an explicit argument needs no environment
    assert (k.gae_bootstrap_truncation, k.gae_tail_value) == (1, 1)
    # the checkpoint's config member carries both; a member written before the fields existed reads as off
    cfg = launch_config(bootstrap_on_truncation=True, bootstrap_tail_value=True, hidden_size=16, depth=1)
    d = dataclasses.asdict(cfg)
    d["action_latency_range"] = list(d["action_latency_range"])
    P = sum(L.param_count(16, 1))
    p = np.arange(P, dtype=np.float32)
    path = str(tmp_path / "ckpt.bin")
    ckpt.save_ckpt(path, p, p, p, 1, 16, 1, dict(num_steps=1), d, {})
    z = ckpt.load_ckpt(path, "config")
    assert z["bootstrap_on_truncation"] is True and z["bootstrap_tail_value"] is True
    z["action_latency_range"] = tuple(z["action_latency_range"])
    assert HumanoidWalkingTaskConfig(**z) == cfg
    old = {k_: v for k_, v in z.items() if k_ not in ("bootstrap_on_truncation", "bootstrap_tail_value")}
    o = HumanoidWalkingTaskConfig(**old)
    assert o.bootstrap_on_truncation is False and o.bootstrap_tail_value is False
