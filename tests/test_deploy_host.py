"""The deployed actor (convert.py init_fn / step_fn), the parts that need no device: the float64 reference pinned against the torch oracle,
the flat carry's size and layout, the inverse of the observation packing, and header / binding agreement on the new ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, constants, layout as L
from tests import deploy_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from kbot_joystick_amd.host import binding
    if not os.path.exists(binding.LIB_PATH):
        binding.build_library()
    return binding.load_library()


def _params(H, depth, seed, scale=3.0):
    """The actor's prefix of kbj_init_params' vector, scaled so the gates leave the linear region; float64."""
    from tests import helpers
    n = L.param_count(H, depth)[0]
    flat = np.zeros(n)
    for name, off, v in helpers.init_params_ref(H, seed, depth):
        if name.startswith("actor."):
            flat[off:off + v.size] = v
    return flat * scale


@pytest.mark.parametrize("H,depth", [(64, 1), (256, 2)])
def test_reference_step_matches_the_torch_oracle(model, H, depth):
    """deploy_ref.step against oracle.nn.net_forward + actor_head + _joint_norm + _encode_pg, both float64, 8 chained steps: two
    independent restatements of convert.py:85-119, so one pins the other."""
    import torch
    from oracle import nn as ON
    n, cfg = 3, L.default_config()
    alpha = float(cfg.lpf_alpha)
    flat = _params(H, depth, 5)
    full = np.zeros(sum(L.param_count(H, depth)))
    full[:flat.size] = flat
    p = ON.unflatten(torch.from_numpy(full), H, depth)
    bias, rng = ON._joint_norm(model, torch.float64)
    gen = np.random.default_rng(1)
    carry = DR.init(n, H, depth)
    hc, lpf = ON.zero_carry(n, H, depth, torch.float64), torch.zeros(n, 20, dtype=torch.float64)

    class Cfg:
        lpf_alpha, min_std, max_std, var_scale = alpha, 0.01, 1.0, 0.5

    for t in range(8):
        ja, jv, pg, gy, cmd = DR.random_sensors(model, gen, n)
        if t == 3:
            cmd[0, :3] = (0.9e-3, 0, 0)
            cmd[1, :3] = (0, 1.1e-3, 0)
        action, carry = DR.step(flat, model, alpha, H, depth, ja, jv, pg, gy, cmd, carry)
        tj, tv, tg, tw, tc = (torch.from_numpy(v).double() for v in (ja, jv, pg, gy, cmd))
        zero = (tc[:, :3].norm(dim=-1) < 1e-3).double()[:, None]
        obs = torch.cat([(tj - bias) / rng, tv / 10.0, ON._encode_pg(tg), tw, zero, tc], -1)
        assert obs.shape == (n, 65) and (t != 3 or (float(zero[0]), float(zero[1])) == (1.0, 0.0))
        out, hc = ON.net_forward(p, "actor", obs, hc, depth)
        y, _, lpf = ON.actor_head(out, obs, lpf, torch.tensor(list(model.joint_bias), dtype=torch.float64), Cfg)
        assert np.abs(action - y.numpy()).max() < 1e-12
        flat_o = np.concatenate([hc[l][k].numpy() for l in range(depth) for k in range(2)] + [lpf.numpy()], -1)
        assert np.abs(carry - flat_o).max() < 1e-12
        assert np.array_equal(carry[:, -20:], action)
    assert np.abs(carry[:, :-20]).max() > 0.5          # the recurrence has left the linear region


def test_carry_size_matches_the_archive(lib, tmp_path):
    from kbot_joystick_amd.host import export
    for H, depth in ((64, 1), (90, 3), (256, 2), (512, 4)):
        cfg = L.default_config(hidden_size=H, depth=depth)
        path = str(tmp_path / f"actor_{H}_{depth}.npz")
        export.export_actor(path, np.zeros(sum(L.param_count(H, depth)), np.float32), H, depth, 0.02, 10.0, 0.01, 1.0, 0.5, np.zeros(20))
        z = np.load(path)
        assert lib.kbj_deploy_carry_size(ctypes.byref(cfg)) == int(z["meta.carry_size"]) == DR.carry_size(H, depth) == depth * 2 * H + 20
    assert lib.kbj_deploy_carry_size(None) < 0 and b"null" in lib.kbj_last_error(None)


def test_flat_carry_round_trip_and_order():
    import torch
    from kbot_joystick_amd.host import deploy
    D, N, H = 3, 5, 24
    g = torch.Generator().manual_seed(0)
    hc, lpf = torch.randn(D, 2, N, H, generator=g), torch.randn(N, 20, generator=g)
    flat = deploy.flat_carry_from((hc, lpf))
    assert flat.shape == (N, D * 2 * H + 20) and flat.is_contiguous()
    assert torch.equal(flat[:, :H], hc[0, 0]) and torch.equal(flat[:, H:2 * H], hc[0, 1]) and torch.equal(flat[:, 2 * H:3 * H], hc[1, 0])
    assert torch.equal(flat[:, -20:], lpf)
    hc2, lpf2 = deploy.carry_from_flat(flat, D, H)
    assert torch.equal(hc2, hc) and torch.equal(lpf2, lpf)
    rows = torch.tensor([3, 1])
    assert torch.equal(deploy.flat_carry_from((hc, lpf), rows), flat[rows])

    class Buf:
        actor_hc, critic_hc = hc, None
    Buf.lpf = lpf
    assert torch.equal(deploy.flat_carry_from(Buf), flat)
    with pytest.raises(Exception):
        deploy.carry_from_flat(flat, D, H + 1)


def test_sensors_from_actor_obs_inverts_the_packing(model):
    """Rows packed by the reference (float64, rounded to float32) -> sensors_from_actor_obs -> the reference's packing again. The sensors
    carry one float32 rounding each, so a column comes back within 2 ulp of the quantity that was rounded, seen through the packing:
      joint position  (q - bias) / range with q rounded at the size of max(|q|, |bias|): 2 spacing(max(|q|, |bias|)) / range, plus the row's own;
      joint velocity  v / 10 with v = 10 x rounded: 2 spacing(|column|);
      roll, pitch, unit vector: functions of a unit vector whose components were rounded at the size of 1; with the tilt below 45 degrees
        atan2's arguments have a norm above 0.7, so an angle moves by less than sqrt(2) x 2^-24 / 0.7 < 2 spacing(1);
      gyroscope, command, zero-command flag: copied, exact."""
    import torch
    from kbot_joystick_amd.host import deploy
    gen = np.random.default_rng(3)
    n = 64
    ja, jv, pg, gy, cmd = DR.random_sensors(model, gen, n)
    cmd[0, :3] = (0.9e-3, 0, 0)
    cmd[1, :3] = (0, 0, 1.1e-3)
    row = DR.pack(model, ja, jv, pg, gy, cmd).astype(np.float32)
    obs = torch.zeros(n, L.LD_ACTOR)
    obs[:, :65] = torch.from_numpy(row)
    sens = [v.numpy() for v in deploy.sensors_from_actor_obs(obs, model)]
    assert [v.shape[1] for v in sens] == [20, 20, 3, 3, 16] and all(v.dtype == np.float32 for v in sens)
    back = DR.pack(model, *sens)
    err = np.abs(back - row.astype(np.float64))
    bias, rng = DR.joint_norm(model)
    sp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    tol = np.zeros_like(err)
    tol[:, 0:20] = 2 * sp(np.maximum(np.abs(sens[0]), np.abs(bias))) / rng + sp(row[:, 0:20])
    tol[:, 20:40] = 2 * sp(row[:, 20:40])
    tol[:, 40:45] = 2 * np.spacing(np.float32(1.0))
    assert (err <= tol).all(), (np.argwhere(err > tol)[:5], float((err / np.maximum(tol, 1e-300)).max()))
    assert np.array_equal(back[:, 45:65], row[:, 45:65].astype(np.float64))            # gyro, cmd_zero, command: exact
    assert (back[0, 48], back[1, 48]) == (1.0, 0.0)
    assert np.array_equal(sens[3], gy) and np.array_equal(sens[4], cmd)
    assert np.abs(sens[0] - ja).max() < 1e-6 and np.abs(sens[1] - jv).max() < 1e-5


def test_header_and_binding_agree_on_the_deploy_abi(lib):
    from kbot_joystick_amd.host import binding
    hdr = open(os.path.join(ROOT, "include", "kbj.h")).read()
    body = re.search(r"typedef struct kbj_deploy_inputs \{(.*?)\} kbj_deploy_inputs;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"const float\*\s*(\w+)\s*;", body)
    assert len(fields) == 5 and len(re.findall(r";", body)) == 5                         # five pointers and nothing else
    assert fields == [n for n, _ in binding.DeployInputs._fields_]
    assert all(t is ctypes.c_void_p for _, t in binding.DeployInputs._fields_)
    assert ctypes.sizeof(binding.DeployInputs) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert tuple(f[:-2] for f in fields) + ("carry",) == constants.STEP_FN_INPUTS         # names and order of convert.py's step_fn
    for name, nargs in (("kbj_deploy_carry_size", 1), ("kbj_deploy_init", 3), ("kbj_deploy_step", 7)):
        assert hasattr(lib, name) and len(binding.SIGNATURES[name][1]) == nargs
        decl = re.search(r"\bint " + name + r"\s*\((.*?)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S).group(1)
        assert len(decl.split(",")) == nargs
    assert "deployment, convert.py" in hdr
