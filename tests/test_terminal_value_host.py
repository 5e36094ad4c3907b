"""The exact terminal value at time-outs (kbj_config.gae_terminal_value) without a device: kbj_check_config, the struct mirror and the three ABI
symbols, the host switch through the environment and a checkpoint, the float64 restatement of the new GAE row (tests/gae_terminal_ref.py)
against tests/gae_ref.py, and the env kernel BODY's terminal critic row in the host emulation (tests/emu/kbj_env_emu_term.cpp) against a twin
whose terminations are switched off."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import gae_ref as G
from tests import gae_terminal_ref as GT
from tests import helpers as H
from tests import terminal_value_cases as TV


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_check_config_and_the_abi():
    """First in the file: fails on a library without the field and the three entries."""
    from kbot_joystick_amd.host import binding
    ok = lambda **kw: binding.check_config(L.default_config(num_envs=64, batch_size=64, **kw))
    assert ok(gae_bootstrap_truncation=1, gae_terminal_value=1) == ""
    assert ok(gae_bootstrap_truncation=1, gae_tail_value=1, gae_terminal_value=1) == ""
    why = ok(gae_bootstrap_truncation=0, gae_terminal_value=1)
    assert "gae_terminal_value" in why and "gae_bootstrap_truncation" in why
    for bad in (2, -1):
        assert "gae_terminal_value" in ok(gae_bootstrap_truncation=1, gae_terminal_value=bad)
    assert "gae_bootstrap_truncation" in ok(gae_bootstrap_truncation=2)                  # what the siblings' tests assert stays
    lib = binding.load_library()
    # one word of the former reserved_f[4]: the struct keeps its size, the field sits right behind terrain_wavelength, three reserved floats follow
    assert lib.kbj_sizeof_config() == C.sizeof(L.Config) and lib.kbj_sizeof_traj() == C.sizeof(binding.Traj)
    f = L.Config
    assert f.gae_terminal_value.offset == f.terrain_wavelength.offset + 4 and f.reserved_f.offset == f.gae_terminal_value.offset + 4
    assert f.reward_scale.offset == f.terrain_wavelength.offset + 4 + 16 and f.reserved_f.size == 12
    assert L.default_config().gae_terminal_value == 0
    for name in ("kbj_env_step_terminal", "kbj_critic_terminal_value", "kbj_set_terminal_values"):
        assert name in binding.SIGNATURES and hasattr(lib, name), name
        assert hasattr(binding.Context, name[4:]), name


def test_config_field_environment_and_checkpoint(tmp_path, monkeypatch):
    from kbot_joystick_amd.host import ckpt
    from kbot_joystick_amd.host.task import HumanoidWalkingTaskConfig, launch_config
    for v in ("KBJ_GAE_TRUNCATION", "KBJ_GAE_TAIL", "KBJ_GAE_TERMINAL"):
        monkeypatch.delenv(v, raising=False)
    assert HumanoidWalkingTaskConfig().bootstrap_terminal_value is False
    assert launch_config().to_kbj(4096).gae_terminal_value == 0
    monkeypatch.setenv("KBJ_GAE_TERMINAL", "1")
    c = launch_config()
    assert c.bootstrap_terminal_value is True and c.bootstrap_on_truncation is False
    with pytest.raises(ValueError, match="bootstrap_on_truncation"):      # implies nothing silently
        c.to_kbj(4096)
    monkeypatch.setenv("KBJ_GAE_TRUNCATION", "1")
    k = launch_config().to_kbj(4096)
    assert (k.gae_bootstrap_truncation, k.gae_tail_value, k.gae_terminal_value) == (1, 0, 1)
    monkeypatch.delenv("KBJ_GAE_TERMINAL"); monkeypatch.delenv("KBJ_GAE_TRUNCATION")
    on = dict(bootstrap_on_truncation=True, bootstrap_terminal_value=True)
    assert launch_config(**on).to_kbj(4096).gae_terminal_value == 1      # an explicit argument needs no environment
    with pytest.raises(ValueError, match="extra_critic_obs") as e:
        launch_config(extra_critic_obs=3, **on).to_kbj(4096)
    assert "bootstrap_terminal_value" in str(e.value)
    with pytest.raises(ValueError, match="record_state"):
        launch_config(record_state=True, **on).to_kbj(4096)
    # the checkpoint's config member carries it; a member written before the field existed reads as off
    cfg = launch_config(hidden_size=16, depth=1, **on)
    d = dataclasses.asdict(cfg)
    d["action_latency_range"] = list(d["action_latency_range"])
    p = np.arange(sum(L.param_count(16, 1)), dtype=np.float32)
    path = str(tmp_path / "ckpt.bin")
    ckpt.save_ckpt(path, p, p, p, 1, 16, 1, dict(num_steps=1), d, {})
    z = ckpt.load_ckpt(path, "config")
    assert z["bootstrap_terminal_value"] is True and z["bootstrap_on_truncation"] is True
    z["action_latency_range"] = tuple(z["action_latency_range"])
    assert HumanoidWalkingTaskConfig(**z) == cfg
    old = {k_: v for k_, v in z.items() if k_ != "bootstrap_terminal_value"}
    assert HumanoidWalkingTaskConfig(**old).bootstrap_terminal_value is False


# ---- the new row of the GAE table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", [(40, 9), (64, 8), (130, 100)])
def test_gae_terminal_reference(N, T):
    p = TV.terminal_problem(N, T)
    done, last = p["done"], p["done"][-1]
    assert (last > 0).sum() >= 1 and (last < 0).sum() >= 1 and (last == 0).sum() >= 1
    for gamma, lam in ((0.94, 0.94), (1.0, 1.0), (float(np.float32(0.94)), float(np.float32(0.94)))):
        for tail in (None, p["tail"]):
            trunc, tt = G.gae_ref(p["value"], p["reward"], done, gamma, lam, 1, tail)
            # value_term := value is the truncation branch itself, operation for operation
            a, t = GT.gae_terminal_ref(p["value"], p["reward"], done, gamma, lam, p["value"], tail)
            assert np.array_equal(a, trunc) and np.array_equal(t, tt)
            # other terminal values: the truncation rows and the rows that chain into them move, nothing else does
            a, t = GT.gae_terminal_ref(p["value"], p["reward"], done, gamma, lam, p["value_term"], tail)
            moved, reach = a != trunc, GT.affected_rows(done)
            assert np.array_equal(moved, reach), (int(moved.sum()), int(reach.sum()))
            assert np.array_equal(t, a + p["value"].astype(np.float64))
            assert reach[done > 0].all() and not reach[done < 0].any() and int(reach.sum()) > int((done > 0).sum())
    # by hand: T = 3, one env, done = [0, +1, 0] and [0, 0, +1]
    g, l, w = 0.9, 0.7, 1.7
    r, v, vt = np.array([0.3, -0.2, 0.5]), np.array([1.1, -0.6, 0.8]), np.array([9.0, 2.5, -4.0])
    a, _ = GT.gae_terminal_ref(v[:, None], r[:, None], np.array([0.0, 1.0, 0.0])[:, None], g, l, vt[:, None], np.array([w]))
    a1 = r[1] + g * vt[1] - v[1]
    assert np.allclose(a[:, 0], [r[0] + g * v[1] - v[0] + g * l * a1, a1, r[2] + g * w - v[2]], rtol=0, atol=1e-15)
    a, _ = GT.gae_terminal_ref(v[:, None], r[:, None], np.array([0.0, 0.0, 1.0])[:, None], g, l, vt[:, None], np.array([w]))
    assert abs(a[2, 0] - (r[2] + g * vt[2] - v[2])) < 1e-15          # a truncation in the last row: the terminal value, not the tail


# ---- the env kernel body: the terminal critic row in the host emulation -------------------------------------------------------------------
EMU_N, EMU_STEPS, EMU_SEED = TV.ENV_N, TV.ENV_STEPS, TV.ENV_SEED


def _emu_terminal_run(model, steps=EMU_STEPS, N=EMU_N, seed=EMU_SEED, solver_newton=1):
    """Teacher-forced from the fp32 oracle's states (the material of helpers.episode_end_run): per step the emulation with the terminal pointer,
    without it, and the twin without terminations, all from the identical state."""
    from oracle import oracle as O
    emu = TV.emu_term_lib()
    cfg, twin = TV.terminal_configs(N, solver_newton)
    o = O.Oracle(model, cfg, seed=seed, precision="f32")
    _, _, x0 = o.reset_all()
    rng = np.random.default_rng(0)
    counts, steps_out = {1: 0, 2: 0, 3: 0}, []

    def run(c, ep0, es0, act, aux_in, ct):
        ep, es, x = ep0.copy(), es0.copy(), aux_in.copy()
        a, cr, n = np.zeros((N, L.LD_ACTOR), np.float32), np.zeros((N, L.LD_CRITIC), np.float32), np.zeros((N, L.AUX["SIZE"]), np.float32)
        emu.kbj_emu_env_step_term(C.byref(model), C.byref(c), C.c_uint32(seed), H.fptr(ep), H.fptr(es), H.fptr(act), H.fptr(x), H.fptr(a), H.fptr(cr), H.fptr(n),
                                  H.fptr(ct) if ct is not None else None)
        return dict(ep=ep, es=es, aux_t=x, actor=a, critic=cr, aux=n)

    for t in range(steps):
        act = np.ascontiguousarray(H.random_actions(model, rng, N), np.float32)
        ep0, es0 = o.ep.copy(), o.es.copy()
        ct = np.full((N, L.LD_CRITIC), TV.SENTINEL, np.float32)
        with_term, plain, off = run(cfg, ep0, es0, act, x0, ct), run(cfg, ep0, es0, act, x0, None), run(twin, ep0, es0, act, x0, None)
        cause = TV.termination_causes(with_term["aux_t"], cfg.unhealthy_z)
        for k in counts:
            counts[k] += int((cause == k).sum())
        steps_out.append(dict(term=with_term, plain=plain, twin=off, rows=ct, cause=cause))
        aux = x0.copy()
        _, _, x0 = o.step(act, aux)
    return dict(counts=dict(height=counts[1], tilt_only=counts[2], timeout=counts[3]), steps=steps_out)


def test_emulated_terminal_rows(model):
    """N = 64, 10 teacher-forced steps of the "episode ends" thresholds (episodes of at most 7 steps). Causes among the compared rows, measured
    on the CPU before the seed was fixed: height 87, tilt only 3, time-out 9 (8 steps: 73 / 3 / 8; 12 steps: 108 / 4 / 11)."""
    run = _emu_terminal_run(model)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    print("terminal rows compared, by cause:", run["counts"])
    assert all(v >= 1 for v in run["counts"].values()), run["counts"]
    for t, s in enumerate(run["steps"]):
        ended = s["cause"] != 0
        # the twin went on from the same state: its next critic row is the observation of the state the episode ended in
        assert (s["twin"]["aux_t"][:, L.AUX["DONE"]] == 0).all(), t
        assert np.array_equal(bits(s["rows"][ended]), bits(s["twin"]["critic"][ended])), t
        assert (s["rows"][ended][:, L.NOBS_CRITIC:] == 0).all(), t                 # the pad column
        assert (bits(s["rows"][~ended]) == bits(np.array([TV.SENTINEL]))[0]).all(), t   # rows of envs that go on are untouched
        # writing the row changed nothing else
        for k in ("ep", "es", "aux_t", "actor", "critic", "aux"):
            assert np.array_equal(bits(s["term"][k]), bits(s["plain"][k])), (t, k)
        # and where an episode ended, the next critic row is NOT the terminal one (the reset has replaced the state)
        if ended.any():
            assert not np.array_equal(bits(s["term"]["critic"][ended]), bits(s["rows"][ended])), t
