"""The deployed actor: convert.py's `init_fn` / `step_fn` (convert.py:74-119) served by ONE HIP launch (csrc/kbj_deploy.h).

What a trained policy is for is the function the robot runs: `step_fn(joint_angles, joint_angular_velocities, projected_gravity, gyroscope,
command, carry) -> (action, carry)` with one flat carry per row. `DeployedActor` runs it on the GPU, from an `export_actor` archive
(host/export.py) or from a live task's parameter tensor, so that an exported policy can be played against the simulator under the contract
the firmware will use. The kinfer / ONNX container itself stays out of scope.

The flat carry of one row is `ravel_pytree(Carry(actor_carry [depth][2][H], lpf [20]))`: for each layer h [H] then c [H], then the 20
low-pass floats. `flat_carry_from` / `carry_from_flat` move between it and the trainer's `[depth][2][N][H]` planes, so a rollout can hand a
running episode to the deployed actor and back. `sensors_from_actor_obs` undoes the packing of an actor observation row.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..spec import compiler, constants, layout as L
from . import binding as B


def _alpha(ctrl_dt: float, cutoff_frequency: float) -> float:
    """ksim.lowpass_one_pole's coefficient, the expression of HumanoidWalkingTaskConfig.to_kbj."""
    return ctrl_dt / (ctrl_dt + 1.0 / (2.0 * math.pi * cutoff_frequency))


def _as_written(x: float) -> float:
    """An archive stores ctrl_dt as the float32 the library's config holds (0.02 -> 0.019999999552965164). The task computed its low-pass
    coefficient from the value as the user wrote it; the shortest decimal that rounds to the stored float32 is that value again."""
    x = float(x)
    return float(np.format_float_positional(np.float32(x), unique=True)) if float(np.float32(x)) == x else x


class DeployedActor:
    """init(n) / step(...) of the deployed policy. Build it with from_archive or from_params."""

    def __init__(self, ctx: B.Context, params: torch.Tensor, device, owns_ctx: bool):
        self.ctx, self.params, self.device, self._owns_ctx = ctx, params, torch.device(device), owns_ctx
        self.hidden_size, self.depth = int(ctx.config.hidden_size), int(ctx.config.depth)
        self.carry_size = ctx.deploy_carry_size()
        if params.numel() < ctx.actor_param_count():
            raise B.KbjError(f"the parameter tensor has {params.numel()} floats, the actor needs {ctx.actor_param_count()}")

    @classmethod
    def from_archive(cls, path: str, device=None, robot: str = "kbot") -> "DeployedActor":
        """An `export_actor` archive -> a deployed actor with a small context of its own (num_envs = 1) built from the archive's meta.*
        (hidden_size, depth, ctrl_dt, cutoff_frequency). `robot`: the compiled model whose joint limits normalise the joint positions; its
        joint biases must be the archive's."""
        if not torch.cuda.is_available():
            raise B.KbjError("DeployedActor needs a HIP device (no CPU fallback)")
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        z = np.load(path)
        H, depth = int(z["meta.hidden_size"]), int(z["meta.depth"])
        if int(z["meta.num_inputs"]) != L.NOBS_ACTOR:
            raise B.KbjError(f"the archive's actor has {int(z['meta.num_inputs'])} inputs; the deployed contract (convert.py:85-105) has {L.NOBS_ACTOR}")
        if tuple(z["meta.step_fn_inputs"]) != constants.STEP_FN_INPUTS:
            raise B.KbjError("the archive's step_fn inputs are not spec/constants.STEP_FN_INPUTS")
        model = compiler.load_model(robot)
        if not np.array_equal(np.asarray(z["meta.joint_biases"], np.float32), np.array(list(model.joint_bias), np.float32)):
            raise B.KbjError(f"the archive's joint biases are not those of robot {robot!r}")
        flat = np.concatenate([np.asarray(z[name], np.float32).reshape(-1) for name, _ in L.param_leaves(H, depth) if name.startswith("actor.")])
        ctrl_dt = _as_written(z["meta.ctrl_dt"])
        cfg = L.default_config(num_envs=1, batch_size=1, hidden_size=H, depth=depth, ctrl_dt=ctrl_dt, lpf_alpha=_alpha(ctrl_dt, float(z["meta.cutoff_frequency"])))
        torch.cuda.set_device(device)
        ctx = B.Context(model, cfg, device.index or 0, torch.cuda.current_stream().cuda_stream)
        return cls(ctx, torch.from_numpy(flat).to(device), device, owns_ctx=True)

    @classmethod
    def from_params(cls, task) -> "DeployedActor":
        """Shares a live task's parameter tensor and context: it always acts with the task's current parameters."""
        return cls(task.ctx, task.params, task.device, owns_ctx=False)

    def init(self, n: int = 1) -> torch.Tensor:
        """init_fn (convert.py:74-82) for n rows: the flat carry [n, carry_size], zeros."""
        carry = torch.empty(n, self.carry_size, device=self.device)
        self.ctx.deploy_init(n, carry)
        return carry

    def step(self, joint_angles, joint_angular_velocities, projected_gravity, gyroscope, command, carry, inplace: bool = False):
        """step_fn (convert.py:84-119): names and order are spec/constants.STEP_FN_INPUTS. Each input is [n, dim] (or [dim] for one row) with
        dims 20, 20, 3, 3, 16 and carry [n, carry_size]; returns (action [n, 20], new carry). inplace: the new carry overwrites `carry`."""
        one = carry.dim() == 1
        ins = []
        for name, x, dim in zip(constants.STEP_FN_INPUTS, (joint_angles, joint_angular_velocities, projected_gravity, gyroscope, command, carry),
                                (L.NU, L.NU, 3, 3, L.NCMD, self.carry_size)):
            x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
            x = x.reshape(1, -1) if x.dim() == 1 else x
            if x.dim() != 2 or x.shape[1] != dim:
                raise B.KbjError(f"{name} must be [n, {dim}], got {tuple(x.shape)}")
            ins.append(x if name == "carry" and inplace else x.contiguous())
        n = ins[-1].shape[0]
        if any(x.shape[0] != n for x in ins):
            raise B.KbjError(f"step_fn inputs disagree on the number of rows: {[x.shape[0] for x in ins]}")
        carry_out = ins[-1] if inplace else torch.empty_like(ins[-1])
        action = torch.empty(n, L.NU, device=self.device)
        self.ctx.deploy_step(self.params, *ins[:5], n, ins[-1], carry_out, action)
        return (action[0], carry_out[0]) if one else (action, carry_out)

    def close(self):
        if self._owns_ctx:
            self.ctx.close()


def _planes(carry_tensors):
    if hasattr(carry_tensors, "actor_hc"):
        return carry_tensors.actor_hc, carry_tensors.lpf
    return carry_tensors


def flat_carry_from(carry_tensors, rows=None) -> torch.Tensor:
    """The trainer's actor carry - `CarryBuffers` or (actor_hc [depth][2][N][H], lpf [N][20]) - as flat rows [n, depth * 2 * H + 20]:
    h of layer 0 first, the low-pass floats last. rows: which envs (index tensor, list or slice), default all."""
    hc, lpf = _planes(carry_tensors)
    rows = slice(None) if rows is None else rows
    hc, lpf = hc[:, :, rows], lpf[rows]
    return torch.cat([hc.permute(2, 0, 1, 3).reshape(hc.shape[2], -1), lpf], dim=1).contiguous()


def carry_from_flat(flat: torch.Tensor, depth: int, hidden_size: int):
    """The inverse: flat rows [n, depth * 2 * H + 20] -> (actor_hc [depth][2][n][H], lpf [n][20])."""
    n, D, H = flat.shape[0], depth, hidden_size
    if flat.shape[1] != 2 * D * H + L.NU:
        raise B.KbjError(f"flat carry rows have {flat.shape[1]} floats, depth {D} x hidden {H} needs {2 * D * H + L.NU}")
    return flat[:, :2 * D * H].reshape(n, D, 2, H).permute(1, 2, 0, 3).contiguous(), flat[:, 2 * D * H:].contiguous()


def sensors_from_actor_obs(actor_obs: torch.Tensor, model) -> tuple:
    """The raw sensors behind packed actor observation rows [..., >= 65], in STEP_FN_INPUTS order (without the carry): joint positions and
    velocities un-normalised, obs[42:45] - the unit projected gravity; the encoding is scale-invariant - as the projected gravity, gyroscope
    and command copied. The inverse of the packing UP TO ROUNDING: each un-normalised value is rounded once to float32, so packing the
    result again reproduces the row to about an ulp of the value, not bit for bit; gyroscope, command and hence the zero-command flag are exact."""
    o = actor_obs
    f32 = lambda v: torch.tensor(list(v), dtype=torch.float32)
    bias, lo, hi = f32(model.joint_bias), f32(model.joint_lo), f32(model.joint_hi)
    rng = torch.maximum(bias - lo, hi - bias)                      # float32, as the kernels form it
    bias, rng = bias.double().to(o.device), rng.double().to(o.device)
    (p0, pn), (v0, vn), (g0, _), (w0, wn), (c0, cn) = L.OBS["JPOS"], L.OBS["JVEL"], L.OBS["PG"], L.OBS["GYRO"], L.OBS["CMD"]
    ja = (o[..., p0:p0 + pn].double() * rng + bias).float()
    jv = (o[..., v0:v0 + vn].double() * L.OBS_JVEL_DIV).float()
    return ja, jv, o[..., g0 + 2:g0 + 5].contiguous(), o[..., w0:w0 + wn].contiguous(), o[..., c0:c0 + cn].contiguous()
