"""CPU tests of the Polak-Ribiere CG constraint solver (kbj_config.solver_newton = 0) in the kernel BODY compiled as a host emulation
(tests/emu), by the acceptance rule of tests/cg_cases.py, and of the host-side selector. The GPU run of the kernels is tests/test_gpu_env_cg.py.

Figures of a run (`-s`) are tabulated in EXPERIMENTS.md "CG solver against the oracle"."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import cg_cases as CG
from tests import helpers as H


def _emu_stepper(solver):
    return lambda model, cfg, seed: H.emu_stepper(model, cfg, seed, lib=H.emu_lib(solver))


@pytest.mark.parametrize("solver,cap", [("reg", 2), ("reg", 3), ("reg", 8), ("reg", 256), ("lds", 3), ("lds", 8)])
def test_cg_steps_match_oracle(solver, cap):
    """The rule on the emulation of the register-resident solver (the product kernel's source, lane by lane) at every cap and of the LDS
    formulation at caps 3 and 8. Without the CG solver the emulation runs Newton whatever the config says and misses the cap-2, cap-3 and
    cap-8 medians by four to five orders of magnitude."""
    CG.run_case("kbot-headless", 256, cap, _emu_stepper(solver), label=f"emu {solver} ")


def test_cg_reset_matches_oracle():
    emu = H.emu_lib()

    def reset(model, cfg, seed):
        N = cfg.num_envs
        ep, es = np.zeros((N, L.EP["SIZE"]), np.float32), np.zeros((N, L.ES["SIZE"]), np.float32)
        a, c, x = np.zeros((N, L.LD_ACTOR), np.float32), np.zeros((N, L.LD_CRITIC), np.float32), np.zeros((N, L.AUX["SIZE"]), np.float32)
        emu.kbj_emu_reset_all(C.byref(model), C.byref(cfg), C.c_uint32(seed), H.fptr(ep), H.fptr(es), H.fptr(a), H.fptr(c), H.fptr(x))
        return ep, es, a, c, x
    CG.reset_case("kbot-headless", 16, reset, exact=True, label="emu ")


def test_solver_field_reaches_config_and_checkpoint(tmp_path, monkeypatch):
    """HumanoidWalkingTaskConfig.solver: "cg" reaches kbj_config.solver_newton beside iterations / ls_iterations, the default is Newton,
    KBJ_SOLVER in the environment moves the default, the name survives the checkpoint's config member, an unknown name is refused."""
    from kbot_joystick_amd.host import ckpt as ckpt_io
    from kbot_joystick_amd.host.task import HumanoidWalkingTaskConfig, launch_config
    monkeypatch.delenv("KBJ_SOLVER", raising=False)
    assert launch_config().solver == "newton" and launch_config().to_kbj(512).solver_newton == 1
    k = launch_config(solver="cg", iterations=3).to_kbj(512)
    assert (k.solver_newton, k.solver_iterations, k.ls_iterations) == (0, 3, 8)
    with pytest.raises(ValueError, match="solver"):
        launch_config(solver="gauss-seidel").to_kbj(512)
    monkeypatch.setenv("KBJ_SOLVER", "cg")
    assert launch_config().solver == "cg" and launch_config().to_kbj(512).solver_newton == 0
    assert launch_config(solver="newton").to_kbj(512).solver_newton == 1          # an explicit choice beats the environment
    monkeypatch.delenv("KBJ_SOLVER")
    # the checkpoint's config member carries the name; a member written before the field existed reads as Newton
    cfg = launch_config(solver="cg", hidden_size=16, depth=1)
    d = dataclasses.asdict(cfg)
    d["action_latency_range"] = list(d["action_latency_range"])
    p = np.arange(sum(L.param_count(16, 1)), dtype=np.float32)
    path = str(tmp_path / "ckpt.bin")
    ckpt_io.save_ckpt(path, p, p, p, 1, 16, 1, dict(num_steps=1), d, {})
    z = ckpt_io.load_ckpt(path, "config")
    assert z["solver"] == "cg"
    z["action_latency_range"] = tuple(z["action_latency_range"])
    assert HumanoidWalkingTaskConfig(**z) == cfg and HumanoidWalkingTaskConfig(**z).to_kbj(512).solver_newton == 0
    assert HumanoidWalkingTaskConfig(**{k_: v for k_, v in z.items() if k_ != "solver"}).solver == "newton"


def test_check_config_accepts_both_solvers():
    """kbj_check_config (host only; kbj_create applies it first): solver_newton 0 and 1 are served, anything else is refused with the reason."""
    from kbot_joystick_amd.host import binding
    why = lambda v: binding.check_config(L.default_config(num_envs=64, batch_size=64, solver_newton=v))
    assert why(1) == "" and why(0) == ""
    for bad in (2, -1):
        assert "solver_newton" in why(bad) and str(bad) in why(bad)
