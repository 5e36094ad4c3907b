"""What tests/test_terminal_value_host.py and tests/test_gpu_terminal_value.py share: the env case of the terminal critic row (configs, the
emulation build, the cause of a termination from its record) and the synthetic GAE problem with terminal values."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from kbot_joystick_amd.spec import layout as L
from tests import gae_ref as G
from tests import helpers as H

# N = 64 envs, 10 teacher-forced steps from the fp32 oracle's states at the "episode ends" thresholds (episodes of at most 7 steps), seed 11.
# Causes among the rows that end, measured with the host emulation before the seed was fixed: Newton height 87, tilt only 3, time-out 9;
# CG the same counts.
ENV_N, ENV_STEPS, ENV_SEED = 64, 10, 11
SENTINEL = np.float32(-7777.25)


def emu_term_lib():
    """tests/emu/kbj_env_emu_term.cpp, compiled the way helpers.emu_lib compiles its neighbour (no sanitizer, nothing preloaded)."""
    out = os.path.join(H.ROOT, "tests", "emu", "_build", "libkbj_emu_term.so")
    src = os.path.join(H.ROOT, "tests", "emu", "kbj_env_emu_term.cpp")
    deps = [src] + [os.path.join(H.ROOT, "kbot-joystick_amd", "csrc", f) for f in ("kbj_env_core.h", "kbj_env_phys.h", "kbj_env_task.h", "kbj_wave.h")]
    deps.append(os.path.join(H.ROOT, "include", "kbj_model.h"))
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-I" + os.path.join(H.ROOT, "include"), "-shared", "-o", out, src])
    return C.CDLL(out)


def terminal_configs(N, solver_newton=1):
    """(cfg, twin): the "episode ends" thresholds with a FIXED command (no command switch can differ between a run that resets and one that goes
    on), and the same with every termination switched off."""
    cfg = H.teacher_forced_config(N, "episode ends")
    cfg.command_mode, cfg.solver_newton = 1, solver_newton
    cfg.fixed_command[0] = 0.5
    twin = L.Config.from_buffer_copy(cfg)
    twin.unhealthy_z, twin.max_tilt_rad, twin.max_episode_steps = float("-inf"), math.pi, 2 ** 30
    return cfg, twin


def termination_causes(aux_t, unhealthy_z):
    """Per env of a completed aux_t record: 0 running, 1 height, 2 tilt only, 3 time-out (the env kernel's own fp32 height expression)."""
    d = aux_t[:, L.AUX["DONE"]]
    low = (aux_t[:, L.AUX["BASEZ"]] - np.minimum(aux_t[:, L.AUX["LFZ"]], aux_t[:, L.AUX["RFZ"]])) < np.float32(unhealthy_z)
    return np.where(d > 0, 3, np.where(d < 0, np.where(low, 1, 2), 0))


def terminal_problem(N, T, seed=0):
    """tests/gae_ref.boundary_problem (all three signs of DONE, the last row included) plus terminal values [T, N]: standard normals where DONE > 0,
    exactly 0 elsewhere - what the value kernel leaves."""
    import torch
    p = G.boundary_problem(N, T, seed)
    g = torch.Generator(device="cpu").manual_seed(4321 + seed)
    p["value_term"] = (torch.randn(T, N, generator=g).numpy() * (p["done"] > 0)).astype(np.float32)
    return p
