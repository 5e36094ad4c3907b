"""ctypes binding of libkbj.so (C ABI: include/kbj.h).

This is the only place the product touches native code. There is NO fallback: if the HIP library is
missing or a call fails, a KbjError is raised. torch is used only as the owner of device memory and
streams (tensor.data_ptr(), torch.cuda.current_stream()).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from ..spec import layout as L

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
LIB_PATH = os.path.join(_CSRC, os.environ.get("KBJ_LIB_NAME", "libkbj.so"))   # KBJ_LIB_NAME: A/B builds of the same ABI (diagnostics)


class KbjError(RuntimeError):
    pass


class Carry(C.Structure):
    _fields_ = [("actor_hc_d", C.c_void_p), ("critic_hc_d", C.c_void_p), ("lpf_d", C.c_void_p),
                ("actor_mirror_hc_d", C.c_void_p), ("critic_mirror_hc_d", C.c_void_p), ("lpf_mirror_d", C.c_void_p)]


class Traj(C.Structure):
    _fields_ = [("T", C.c_int32), ("N", C.c_int32),
                ("actor_obs_d", C.c_void_p), ("critic_obs_d", C.c_void_p), ("aux_d", C.c_void_p),
                ("action_d", C.c_void_p), ("logp_d", C.c_void_p), ("value_d", C.c_void_p), ("reward_d", C.c_void_p),
                ("carry0_actor_hc_d", C.c_void_p), ("carry0_critic_hc_d", C.c_void_p), ("carry0_lpf_d", C.c_void_p),
                ("carry0_actor_mirror_hc_d", C.c_void_p), ("carry0_critic_mirror_hc_d", C.c_void_p),
                ("carry0_lpf_mirror_d", C.c_void_p), ("reward_comps_d", C.c_void_p), ("qstate_d", C.c_void_p), ("value_tail_d", C.c_void_p)]


class PpoVars(C.Structure):
    _fields_ = [("logp_d", C.c_void_p), ("value_d", C.c_void_p), ("entropy_d", C.c_void_p), ("action_std_d", C.c_void_p), ("action_mean_d", C.c_void_p)]


class DeployInputs(C.Structure):
    """kbj_deploy_inputs: the raw sensor arrays of convert.py's step_fn (spec/constants.STEP_FN_INPUTS without the carry), N rows each."""
    _fields_ = [("joint_angles_d", C.c_void_p), ("joint_angular_velocities_d", C.c_void_p), ("projected_gravity_d", C.c_void_p),
                ("gyroscope_d", C.c_void_p), ("command_d", C.c_void_p)]


class PushCriteria(C.Structure):
    """kbj_push_criteria: the tolerance of each tracking error (layout.TERR order; +inf ignores a column), the rows a recovery must hold and
    the rows behind the push that are watched."""
    _fields_ = [("tol", C.c_float * L.NTERR), ("hold_steps", C.c_int32), ("window_steps", C.c_int32)]


class StepCriteria(C.Structure):
    """kbj_step_criteria: per channel (forward, sideways, yaw) the smallest command change that makes it active and the floor of its settle
    band, the band as a share of the step, the rise level in (0, 1], the rows of the smoothing window (1..32), the rows a settled run must
    hold and the rows behind the step that are watched. Settings of the caller, not measured thresholds."""
    _fields_ = [("min_step", C.c_float * L.NSCH), ("band_abs", C.c_float * L.NSCH), ("band_frac", C.c_float), ("rise_level", C.c_float),
                ("smooth_steps", C.c_int32), ("hold_steps", C.c_int32), ("window_steps", C.c_int32)]


class FrequencyCriteria(C.Structure):
    """kbj_frequency_criteria: per channel (forward, sideways, yaw) the smallest swing of the driven command word over the measured window
    that counts as a moved stick. A setting of the caller, not a measured threshold."""
    _fields_ = [("min_amp", C.c_float * L.NSCH)]


class ActuatorLevels(C.Structure):
    """kbj_actuator_levels: per actuator (spec/constants.JOINT_NAMES order) the torque level (N m), the speed level (rad/s, +inf counts
    nothing) and the joint-stop band (rad). Settings of the caller (host/actuator.py actuator_levels), not figures of the reference."""
    _fields_ = [("tau_level", C.c_float * L.NU), ("vel_level", C.c_float * L.NU), ("pos_lo", C.c_float * L.NU), ("pos_hi", C.c_float * L.NU)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("launches", C.c_int32), ("total_ms", C.c_float), ("flops", C.c_double)]


# every struct the two headers define: C name -> its mirror
STRUCTS = {
    "kbj_model": L.Model, "kbj_config": L.Config, "kbj_carry": Carry, "kbj_traj": Traj, "kbj_ppo_vars": PpoVars,
    "kbj_deploy_inputs": DeployInputs, "kbj_push_criteria": PushCriteria, "kbj_step_criteria": StepCriteria,
    "kbj_frequency_criteria": FrequencyCriteria, "kbj_actuator_levels": ActuatorLevels, "kbj_kernel_stat": KernelStat,
}

_vp, _i, _u32, _f, _sz = C.c_void_p, C.c_int, C.c_uint32, C.c_float, C.c_size_t
_cfgp = C.POINTER(L.Config)

# every symbol include/kbj.h declares: name -> (restype, argtypes). A new entry point needs its entry here (a new struct its entry in
# STRUCTS) and no test of its own: tests/test_abi_mirror.py takes the arity and every argument's type of each entry, and every field of
# each struct, from the header through the host compiler, and refuses a declaration of the header that has no entry.
SIGNATURES = {
    "kbj_create": (_i, [C.POINTER(_vp), _vp, _sz, _cfgp, _i, _vp]),
    "kbj_destroy": (_i, [_vp]),
    "kbj_last_error": (C.c_char_p, [_vp]),
    "kbj_check_config": (_i, [_vp, _vp, _sz]),
    "kbj_set_advantage_sums": (_i, [_vp, _vp]),
    "kbj_ppo_prefetch": (_i, [_vp, _vp, _vp]),
    "kbj_sizeof_model": (_i, []),
    "kbj_sizeof_config": (_i, []),
    "kbj_sizeof_traj": (_i, []),
    "kbj_sizeof_carry": (_i, []),
    "kbj_sizeof_step_criteria": (_i, []),
    "kbj_sizeof_frequency_criteria": (_i, []),
    "kbj_synchronize": (_i, [_vp]),
    "kbj_env_reset_all": (_i, [_vp, _u32, _vp, _vp, _vp]),
    "kbj_env_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "kbj_env_step_terminal": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kbj_env_record_state": (_i, [_vp, _vp]),
    "kbj_env_reset_where": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "kbj_env_set_command": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "kbj_env_set_push": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "kbj_env_perturb": (_i, [_vp, _vp, _vp, _vp]),
    "kbj_env_get_qstate": (_i, [_vp, _vp, _vp]),
    "kbj_env_set_qstate": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kbj_env_get_state": (_i, [_vp, _vp, _vp]),
    "kbj_env_set_state": (_i, [_vp, _vp, _vp]),
    "kbj_env_get_reward_carry": (_i, [_vp, _vp]),
    "kbj_env_set_reward_carry": (_i, [_vp, _vp]),
    "kbj_rewards": (_i, [_vp, _vp, _i, _vp, _vp]),
    "kbj_param_count": (_sz, [_cfgp]),
    "kbj_actor_param_count": (_sz, [_cfgp]),
    "kbj_init_params": (_i, [_vp, _u32, _vp]),
    "kbj_mirror_table": (_i, [_vp, _sz, _i, _vp, _vp, _vp]),
    "kbj_policy_step": (_i, [_vp, _vp, _vp, _vp, C.POINTER(Carry), _u32, _u32, _i, _vp, _vp, _vp]),
    "kbj_carry_reset": (_i, [_vp, C.POINTER(Carry), _vp, _i]),
    "kbj_critic_value": (_i, [_vp, _vp, _vp, C.POINTER(Carry), _vp]),
    "kbj_critic_terminal_value": (_i, [_vp, _vp, _vp, C.POINTER(Carry), _vp, _i, _vp]),
    "kbj_set_terminal_values": (_i, [_vp, _vp]),
    "kbj_deploy_carry_size": (_i, [_cfgp]),
    "kbj_deploy_init": (_i, [_vp, _i, _vp]),
    "kbj_deploy_step": (_i, [_vp, _vp, C.POINTER(DeployInputs), _i, _vp, _vp, _vp]),
    "kbj_rollout": (_i, [_vp, _vp, C.POINTER(Carry), _u32, _u32, C.POINTER(Traj)]),
    "kbj_set_rollout_argmax": (_i, [_vp, _i]),
    "kbj_recurrence_residency": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "kbj_gae": (_i, [_vp, C.POINTER(Traj), _vp, _vp]),
    "kbj_episode_stats": (_i, [_vp, C.POINTER(Traj), _vp, _vp]),
    "kbj_tracking_stats": (_i, [_vp, C.POINTER(Traj), _i, _vp, _vp, _vp]),
    "kbj_gait_stats": (_i, [_vp, C.POINTER(Traj), _vp, _vp, _vp]),
    "kbj_actuator_stats": (_i, [_vp, C.POINTER(Traj), C.POINTER(ActuatorLevels), _vp, _vp, _vp]),
    "kbj_push_recovery": (_i, [_vp, C.POINTER(Traj), _vp, _vp, C.POINTER(PushCriteria), _vp, _vp, _i, _vp]),
    "kbj_step_response": (_i, [_vp, C.POINTER(Traj), _vp, C.POINTER(StepCriteria), _vp, _vp, _vp, _i, _vp]),
    "kbj_frequency_response": (_i, [_vp, C.POINTER(Traj), _vp, C.POINTER(FrequencyCriteria), _vp, _vp, _vp, _i, _vp]),
    "kbj_robustness": (_i, [_vp, C.POINTER(Traj), _vp, _vp, _vp, _i, _vp]),
    "kbj_ppo_grad": (_i, [_vp, _vp, C.POINTER(Traj), _vp, _i, _vp, _vp, _vp, _vp]),
    "kbj_ppo_forward": (_i, [_vp, _vp, C.POINTER(Traj), _vp, _i, C.POINTER(PpoVars)]),
    "kbj_stream_wait_actor_grad": (_i, [_vp, _vp]),
    "kbj_adamw_step": (_i, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _f]),
    "kbj_set_learning_rate": (_i, [_vp, _f]),
    "kbj_profile_begin": (_i, [_vp]),
    "kbj_profile_end": (_i, [_vp, C.POINTER(_f), C.POINTER(_i), C.POINTER(_f), C.POINTER(_i)]),
    "kbj_profile_kernel_stats": (_i, [_vp, C.POINTER(KernelStat), _i, C.POINTER(_i)]),
}


def build_library(force: bool = False) -> str:
    """Compile libkbj.so for gfx950 with hipcc (works without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", _CSRC, "-s", "-j4"])
    return LIB_PATH


_lib = None


def load_library_at(path: str) -> C.CDLL:
    """dlopen one build of the ABI (RTLD_LOCAL: several builds can live in one process, e.g. the A/B solver test) and type its symbols."""
    if not os.path.exists(path):
        raise KbjError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch bundles its own ROCm runtime: import it first so that libkbj.so binds to the SAME libamdhip64
    # (loading /opt/rocm's copy first leaves the process with two HIP runtimes and no visible device)
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here means the library does not match include/kbj.h
        fn.restype, fn.argtypes = res, args
    return lib


def load_library() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = load_library_at(LIB_PATH)
    return _lib


def check_config(cfg) -> str:
    """kbj_check_config (host-only): '' when the library serves this kbj_config, else the reason kbj_create would refuse it with."""
    why = C.create_string_buffer(512)
    rc = load_library().kbj_check_config(C.addressof(cfg), why, C.sizeof(why))
    return "" if rc == 0 else why.value.decode()


def mirror_table(model, critic: bool):
    """kbj_mirror_table: (src, mul, add) arrays of the packed-row mirror the kernels apply (host-only call, no device needed)."""
    import numpy as np
    n = L.LD_CRITIC if critic else L.LD_ACTOR
    src, mul, add = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    rc = load_library().kbj_mirror_table(C.addressof(model), C.sizeof(model), int(critic), src.ctypes.data, mul.ctypes.data, add.ctypes.data)
    if rc != n:
        raise KbjError(f"kbj_mirror_table returned {rc}, expected {n}")
    return src, mul, add


def _ptr(t):
    """Device/host pointer of a torch tensor or numpy array (must be contiguous)."""
    if t is None or isinstance(t, int):   # an int is a raw address (e.g. a column inside a row-major tensor)
        return t
    if hasattr(t, "data_ptr"):
        if not t.is_contiguous():
            raise KbjError("tensor passed to libkbj must be contiguous")
        return t.data_ptr()
    return t.ctypes.data


class Context:
    """RAII wrapper of kbj_ctx."""

    def __init__(self, model: L.Model, config: L.Config, device: int = 0, stream: int | None = None, lib: C.CDLL | None = None):
        self._h = _vp()                    # first: close() / __del__ read it whatever fails below
        self.lib = lib if lib is not None else load_library()
        if self.lib.kbj_sizeof_model() != C.sizeof(L.Model) or self.lib.kbj_sizeof_config() != C.sizeof(L.Config):
            raise KbjError("struct layout mismatch between spec/layout.py and libkbj.so")
        if self.lib.kbj_sizeof_traj() != C.sizeof(Traj) or self.lib.kbj_sizeof_carry() != C.sizeof(Carry):
            raise KbjError("struct layout mismatch between host/binding.py (Traj / Carry) and libkbj.so")
        self.model, self.config = model, config
        blob = C.string_at(C.addressof(model), C.sizeof(model))
        rc = self.lib.kbj_create(C.byref(self._h), blob, len(blob), C.byref(config), device, stream)
        if rc != 0:
            raise KbjError(self.lib.kbj_last_error(None).decode())

    def close(self):
        if self._h.value:
            self.lib.kbj_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, name: str, *args):
        rc = getattr(self.lib, name)(self._h, *args)
        if rc != 0:
            raise KbjError(f"{name}: {self.lib.kbj_last_error(self._h).decode()}")

    # ---- thin typed helpers ----
    def synchronize(self):
        self.call("kbj_synchronize")

    def env_reset_all(self, seed, actor0, critic0, aux0):
        self.call("kbj_env_reset_all", seed, _ptr(actor0), _ptr(critic0), _ptr(aux0))

    def env_step(self, action, aux_t, actor_next, critic_next, aux_next, qstate_t=None):
        """qstate_t: optional [N][QSTATE SIZE] row that receives the step's state record (kbj_env_record_state, one-shot)."""
        if qstate_t is not None:
            self.call("kbj_env_record_state", _ptr(qstate_t))
        self.call("kbj_env_step", _ptr(action), _ptr(aux_t), _ptr(actor_next), _ptr(critic_next), _ptr(aux_next))

    def env_step_terminal(self, action, aux_t, actor_next, critic_next, aux_next, critic_term):
        """kbj_env_step_terminal: env_step, and for the envs whose episode ends in this step their terminal critic row (the state before the
        reset) into critic_term [N, ld_critic]; rows of envs that go on are not written."""
        self.call("kbj_env_step_terminal", _ptr(action), _ptr(aux_t), _ptr(actor_next), _ptr(critic_next), _ptr(aux_next), _ptr(critic_term))

    def env_reset_where(self, mask, actor_next, critic_next, aux_next):
        self.call("kbj_env_reset_where", _ptr(mask), _ptr(actor_next), _ptr(critic_next), _ptr(aux_next))

    def env_set_command(self, mask, cmd, actor_next, critic_next, aux_next):
        """mask None = every env; cmd [N, 16] float32 on the device."""
        self.call("kbj_env_set_command", _ptr(mask) if mask is not None else None, _ptr(cmd), _ptr(actor_next), _ptr(critic_next), _ptr(aux_next))

    def env_set_push(self, mask, wrench, steps, next=None):
        """kbj_env_set_push: for the envs of mask [N] float32 (None = every env) the push wrench [N, 6] (force, torque; world frame), the control
        steps it is applied for [N] and, with `next` [N], the control steps until the built-in event draws again (layout.PUSH_NEVER: never);
        float32 device tensors. Asynchronous; no observation row changes."""
        self.call("kbj_env_set_push", _ptr(mask), _ptr(wrench), _ptr(steps), _ptr(next))

    def env_perturb(self, mask, pert, status=None):
        """kbj_env_perturb: for the envs of mask [N] float32 (None = every env) the physics and actuator columns of the model row rewritten from
        the model's nominal values and pert [N, PERT SIZE] float32 (layout.PERT); status None or [N] int32, overwritten for every env (0 not
        masked, 1 written, -1 refused: an invalid record leaves its row alone); device tensors. Asynchronous; no observation row changes."""
        self.call("kbj_env_perturb", _ptr(mask), _ptr(pert), _ptr(status))

    def env_get_qstate(self, qpos, qvel):
        """kbj_env_get_qstate: every env's qpos [N, 27] / qvel [N, 26] into device tensors (asynchronous)."""
        self.call("kbj_env_get_qstate", _ptr(qpos), _ptr(qvel))

    def env_set_qstate(self, mask, qpos, qvel, actor_next, critic_next, aux_next):
        """kbj_env_set_qstate: new qpos / qvel for the masked envs (None = all) + their next observation rows rewritten."""
        self.call("kbj_env_set_qstate", _ptr(mask) if mask is not None else None, _ptr(qpos), _ptr(qvel), _ptr(actor_next), _ptr(critic_next), _ptr(aux_next))

    def env_get_state(self):
        import numpy as np
        N = self.config.num_envs
        ep = np.zeros((N, L.EP["SIZE"]), np.float32)
        es = np.zeros((N, L.ES["SIZE"]), np.float32)
        self.call("kbj_env_get_state", _ptr(ep), _ptr(es))
        return ep, es

    def env_set_state(self, ep, es):
        import numpy as np
        ep = None if ep is None else np.ascontiguousarray(ep, np.float32)
        es = None if es is None else np.ascontiguousarray(es, np.float32)
        self.call("kbj_env_set_state", _ptr(ep), _ptr(es))

    def env_get_reward_carry(self):
        import numpy as np
        rc = np.zeros((self.config.num_envs, L.RC["SIZE"]), np.float32)
        self.call("kbj_env_get_reward_carry", _ptr(rc))
        return rc

    def env_set_reward_carry(self, rc):
        import numpy as np
        rc = np.ascontiguousarray(rc, np.float32)
        if rc.shape != (self.config.num_envs, L.RC["SIZE"]):
            raise KbjError(f"reward carry must be [{self.config.num_envs}][{L.RC['SIZE']}], got {rc.shape}")
        self.call("kbj_env_set_reward_carry", _ptr(rc))

    def rewards(self, aux, T, reward, comps=None):
        self.call("kbj_rewards", _ptr(aux), T, _ptr(reward), _ptr(comps))

    def param_count(self) -> int:
        return int(self.lib.kbj_param_count(C.byref(self.config)))

    def actor_param_count(self) -> int:
        return int(self.lib.kbj_actor_param_count(C.byref(self.config)))

    def init_params(self, seed, params):
        self.call("kbj_init_params", seed, _ptr(params))

    def policy_step(self, params, actor_obs, critic_obs, carry: Carry, seed, step_index, argmax, action, logp, value):
        self.call("kbj_policy_step", _ptr(params), _ptr(actor_obs), _ptr(critic_obs), C.byref(carry), seed, step_index,
                  int(argmax), _ptr(action), _ptr(logp), _ptr(value))

    def carry_reset(self, carry: Carry, done, stride):
        self.call("kbj_carry_reset", C.byref(carry), _ptr(done), stride)

    def critic_value(self, params, critic_obs, carry: Carry, value):
        """kbj_critic_value: the critic's value [N] of ONE observation row [N, ld_critic] from the critic carries in `carry`; no carry advances.
        Needs a context with kbj_config.gae_tail_value = 1."""
        self.call("kbj_critic_value", _ptr(params), _ptr(critic_obs), C.byref(carry), _ptr(value))

    def critic_terminal_value(self, params, critic_term, carry: Carry, done, stride, value_term):
        """kbj_critic_terminal_value: value_term [N] = the critic's value of the terminal rows critic_term [N, ld_critic] from the un-reset
        critic carries where done (base pointer + stride in floats, as carry_reset takes it) > 0, exactly 0 elsewhere; nothing else is written."""
        self.call("kbj_critic_terminal_value", _ptr(params), _ptr(critic_term), C.byref(carry), _ptr(done), stride, _ptr(value_term))

    def set_terminal_values(self, value_term):
        """kbj_set_terminal_values: the [T, N] float32 device tensor the following rollout() calls write and gae() calls read
        (kbj_config.gae_terminal_value), or None. The caller keeps it alive."""
        self.call("kbj_set_terminal_values", _ptr(value_term))

    def deploy_carry_size(self) -> int:
        """kbj_deploy_carry_size: floats of one row's flat carry (depth * 2 * hidden_size + 20, convert.py:71)."""
        return int(self.lib.kbj_deploy_carry_size(C.byref(self.config)))

    def deploy_init(self, n: int, carry):
        """kbj_deploy_init (convert.py init_fn): zeros into carry [n, carry_size]."""
        self.call("kbj_deploy_init", int(n), _ptr(carry))

    def deploy_step(self, actor_params, joint_angles, joint_angular_velocities, projected_gravity, gyroscope, command, n: int, carry_in, carry_out, action):
        """kbj_deploy_step (convert.py step_fn) for n rows: raw sensors + flat carry -> action [n, 20] + new flat carry (carry_out may be carry_in)."""
        inp = DeployInputs(_ptr(joint_angles), _ptr(joint_angular_velocities), _ptr(projected_gravity), _ptr(gyroscope), _ptr(command))
        self.call("kbj_deploy_step", _ptr(actor_params), C.byref(inp), int(n), _ptr(carry_in), _ptr(carry_out), _ptr(action))

    def rollout(self, params, carry: Carry, seed, first_step_index, traj: Traj):
        self.call("kbj_rollout", _ptr(params), C.byref(carry), seed, first_step_index, C.byref(traj))

    def set_rollout_argmax(self, argmax: bool):
        """kbj_set_rollout_argmax: the following rollout() calls act with the distribution's mode (validation rollouts)."""
        self.call("kbj_set_rollout_argmax", int(bool(argmax)))

    def recurrence_residency(self):
        """kbj_recurrence_residency: (workgroups of one persistent recurrence launch, launches in flight at once, resident workgroup slots)."""
        g, c, s = _i(0), _i(0), _i(0)
        self.call("kbj_recurrence_residency", C.byref(g), C.byref(c), C.byref(s))
        return g.value, c.value, s.value

    def gae(self, traj: Traj, adv, target):
        self.call("kbj_gae", C.byref(traj), _ptr(adv), _ptr(target))

    def episode_stats(self, traj: Traj, acc, stats):
        """kbj_episode_stats: acc [N, EACC SIZE] float32 (updated in place), stats [EPST SIZE] float64 (overwritten), both on the device."""
        self.call("kbj_episode_stats", C.byref(traj), _ptr(acc), _ptr(stats))

    def tracking_stats(self, traj: Traj, settle_steps: int, acc, stats, err=None):
        """kbj_tracking_stats: acc [N, TACC SIZE] float32 (updated in place), stats [TRK SIZE] float64 (overwritten), err None or
        [T, N, TERR SIZE] float32 (every row's errors, mode, settled flag, since), all on the device."""
        self.call("kbj_tracking_stats", C.byref(traj), int(settle_steps), _ptr(acc), _ptr(stats), _ptr(err))

    def gait_stats(self, traj: Traj, acc, stats, env=None):
        """kbj_gait_stats: acc [N, GACC SIZE] float32 (updated in place), stats [GAIT SIZE] float64 (overwritten), env None or
        [N, GENV SIZE] float32 (every env's totals of this call, overwritten), all on the device."""
        self.call("kbj_gait_stats", C.byref(traj), _ptr(acc), _ptr(stats), _ptr(env))

    def actuator_stats(self, traj: Traj, levels: ActuatorLevels, acc, stats, env=None):
        """kbj_actuator_stats: levels an ActuatorLevels (host), acc [N, AACC SIZE] float32 (updated in place), stats [ACT SIZE] float64
        (overwritten), env None or [N, AENV SIZE] float32 (every env's totals of this call, overwritten), all on the device. The
        trajectory needs its state record (qstate_d)."""
        self.call("kbj_actuator_stats", C.byref(traj) if traj is not None else None, C.byref(levels) if levels is not None else None, _ptr(acc), _ptr(stats), _ptr(env))

    def push_recovery(self, traj: Traj, err, sched, criteria: PushCriteria, rec, group=None, G: int = 1, stats=None):
        """kbj_push_recovery: err [T, N, TERR SIZE] float32 (kbj_tracking_stats' per-row output), sched [N, 2] int32 (start row, pushed steps;
        start < 0: no push), rec [N, PREC SIZE] float32 (overwritten), group None or [N] int32 in [0, G), stats None or [G, PSTAT SIZE]
        float64 (overwritten), all on the device."""
        self.call("kbj_push_recovery", C.byref(traj), _ptr(err), _ptr(sched), C.byref(criteria) if criteria is not None else None, _ptr(rec), _ptr(group), int(G), _ptr(stats))

    def step_response(self, traj: Traj, sched, criteria: StepCriteria, sig, rec, group=None, G: int = 1, stats=None):
        """kbj_step_response: sched [N] int32 (the first row of the new command; < 0: no step), sig [T, N, SSIG SIZE] float32 and rec
        [N, SREC SIZE] float32 (both overwritten), group None or [N] int32 in [0, G), stats None or [G, SSTAT SIZE] float64 (overwritten),
        all on the device."""
        self.call("kbj_step_response", C.byref(traj) if traj is not None else None, _ptr(sched), C.byref(criteria) if criteria is not None else None, _ptr(sig), _ptr(rec),
                  _ptr(group), int(G), _ptr(stats))

    def frequency_response(self, traj: Traj, sched, criteria: FrequencyCriteria, sig, rec, group=None, G: int = 1, stats=None):
        """kbj_frequency_response: sched [N, 4] int32 (first measured row, period in rows, driven channel, whole periods; row < 0: no window),
        sig [T, N, SSIG SIZE] float32 and rec [N, FREC SIZE] float64 (both overwritten), group None or [N] int32 in [0, G), stats None or
        [G, FSTAT SIZE] float64 (overwritten), all on the device."""
        self.call("kbj_frequency_response", C.byref(traj) if traj is not None else None, _ptr(sched), C.byref(criteria) if criteria is not None else None, _ptr(sig), _ptr(rec),
                  _ptr(group), int(G), _ptr(stats))

    def robustness(self, traj: Traj, err, rec, group=None, G: int = 1, stats=None):
        """kbj_robustness: err [T, N, TERR SIZE] float32 (kbj_tracking_stats' per-row output), rec [N, RREC SIZE] float64 (overwritten), group
        None or [N] int32 in [0, G), stats None or [G, RSTAT SIZE] float64 (overwritten), all on the device."""
        self.call("kbj_robustness", C.byref(traj) if traj is not None else None, _ptr(err), _ptr(rec), _ptr(group), int(G), _ptr(stats))

    def ppo_grad(self, params, traj: Traj, env_idx, B, adv, target, grad, metrics):
        self.call("kbj_ppo_grad", _ptr(params), C.byref(traj), _ptr(env_idx), B, _ptr(adv), _ptr(target), _ptr(grad),
                  _ptr(metrics))

    def ppo_forward(self, params, traj: Traj, env_idx, B, logp, value, entropy=None, action_std=None, action_mean=None):
        """kbj_ppo_forward: the on-policy pass (no gradients) for the B envs `env_idx` names; outputs are [T][B](x20) in env_idx order."""
        out = PpoVars(_ptr(logp), _ptr(value), _ptr(entropy), _ptr(action_std), _ptr(action_mean))
        self.call("kbj_ppo_forward", _ptr(params), C.byref(traj), _ptr(env_idx), B, C.byref(out))

    def ppo_prefetch(self, traj: "Traj", env_idx):
        """kbj_ppo_prefetch: queue the parameter-independent gathers of the NEXT ppo_grad (same traj / env_idx pointers) now."""
        self.call("kbj_ppo_prefetch", C.byref(traj), _ptr(env_idx))

    def set_advantage_sums(self, sums):
        """kbj_set_advantage_sums: a float64 [3] device tensor (sum adv, sum adv^2, count) or None (default: each minibatch's own)."""
        self.call("kbj_set_advantage_sums", _ptr(sums))

    def stream_wait_actor_grad(self, hip_stream: int):
        self.call("kbj_stream_wait_actor_grad", hip_stream)

    def adamw_step(self, params, m, v, grad, step, grad_scale=1.0):
        self.call("kbj_adamw_step", _ptr(params), _ptr(m), _ptr(v), _ptr(grad), step, grad_scale)

    def set_learning_rate(self, lr: float):
        self.call("kbj_set_learning_rate", lr)

    def profile_begin(self):
        self.call("kbj_profile_begin")

    def profile_end(self):
        a, b, c, d = _f(), _i(), _f(), _i()
        self.call("kbj_profile_end", C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        arr, n = (KernelStat * 32)(), _i()
        self.call("kbj_profile_kernel_stats", arr, 32, C.byref(n))
        kernels = [dict(name=arr[k].name.decode(), launches=arr[k].launches, total_ms=arr[k].total_ms, flops=arr[k].flops) for k in range(n.value)]
        return dict(env_step_ms=a.value, env_step_launches=b.value, nn_ms=c.value, nn_launches=d.value, kernels=kernels)
