"""The one exchange step of the hot path: sum-all-reduce of the flat fp32 gradient over the data-parallel ranks
(RCCL over xGMI on the GPU job, gloo in the CPU tests). The 1/world scale is applied inside kbj_adamw_step."""
from __future__ import annotations

import numpy as np
import torch

from ..spec import layout as L


def env_shard(num_envs_total: int, rank: int, world_size: int) -> tuple[int, int]:
    """(num_envs_local, env_id_offset): rank r owns global env ids [r*N, (r+1)*N) so that every env's RNG streams
    (threefry key = (seed, global env id)) are independent of the number of GPUs."""
    if num_envs_total % world_size != 0:
        raise ValueError("num_envs must be divisible by the number of ranks")
    n = num_envs_total // world_size
    return n, rank * n


FORCE_COLLECTIVE = False      # run the collective even at world_size 1 (tests: the RCCL leg on a one-GPU box)
TIMING = None                 # set to a list to collect (start, end) CUDA event pairs around every gradient all-reduce (bench.py)


def allreduce_grad_overlapped_(ctx, grad: torch.Tensor, n_actor: int, world_size: int, comm_stream) -> float:
    """The same exchange in two pieces: the actor's slice grad[:n_actor] on `comm_stream` as soon as kbj_ppo_grad has finished it
    (kbj_stream_wait_actor_grad: ~0.5 ms before the critic's), the critic's slice on the current stream behind the whole call; the
    current stream then waits for `comm_stream`. Same sums, same result as allreduce_grad_."""
    if world_size > 1 or FORCE_COLLECTIVE:
        import torch.distributed as dist
        ctx.stream_wait_actor_grad(comm_stream.cuda_stream)
        with torch.cuda.stream(comm_stream):
            dist.all_reduce(grad[:n_actor], op=dist.ReduceOp.SUM)
        dist.all_reduce(grad[n_actor:], op=dist.ReduceOp.SUM)
        torch.cuda.current_stream().wait_stream(comm_stream)
    return 1.0 / world_size


def allreduce_grad_(grad: torch.Tensor, world_size: int) -> float:
    """In-place SUM all-reduce on the current stream; returns the scale (1/world) the optimizer step must apply."""
    if world_size > 1 or FORCE_COLLECTIVE:
        import torch.distributed as dist
        if TIMING is not None and grad.is_cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dist.all_reduce(grad, op=dist.ReduceOp.SUM)
            e1.record()
            TIMING.append((e0, e1))
        else:
            dist.all_reduce(grad, op=dist.ReduceOp.SUM)
    return 1.0 / world_size


def global_advantage_sums(adv_minibatch: torch.Tensor, world_size: int) -> torch.Tensor:
    """(sum adv, sum adv^2, count) of the GLOBAL minibatch as three float64 on the tensor's device: this rank's sums all-reduced over the
    data-parallel ranks. Fed to kbj_set_advantage_sums (product) / ppo_loss(adv_sums=...) (oracle): every rank then
    normalises its advantages with the same mean and variance, and the averaged gradient equals the single-process gradient of the union."""
    a = adv_minibatch.to(torch.float64)
    sums = torch.stack([a.sum(), (a * a).sum(), torch.tensor(float(a.numel()), dtype=torch.float64, device=a.device)])
    if world_size > 1 or FORCE_COLLECTIVE:
        import torch.distributed as dist
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
    return sums


# kbj_episode_stats vectors (kbj_model.h KBJ_EPST_*): every slot is a count or a sum over the finished episodes, except these three
_EPST_MIN, _EPST_MAX, _EPST_LENGTH_MAX = L.EPST["RETURN_MIN"], L.EPST["RETURN_MAX"], L.EPST["LENGTH_MAX"]


def empty_episode_stats() -> np.ndarray:
    """The KBJ_EPST vector of no finished episode: zeros, RETURN_MIN = +inf, RETURN_MAX = -inf."""
    v = np.zeros(L.EPST["SIZE"], np.float64)
    v[_EPST_MIN], v[_EPST_MAX] = np.inf, -np.inf
    return v


def combine_episode_stats(vectors) -> np.ndarray:
    """Statistics of the union of the episode sets that the given KBJ_EPST vectors describe (other ranks' envs, or later rollouts): counts
    and sums add up in list order, in float64; minimum, maximum and longest episode are taken over the list. Pure host arithmetic, the same
    that reduce_episode_stats performs with collectives."""
    out = empty_episode_stats()
    for v in vectors:
        v = np.asarray(v, np.float64)
        lo, hi, longest = min(out[_EPST_MIN], v[_EPST_MIN]), max(out[_EPST_MAX], v[_EPST_MAX]), max(out[_EPST_LENGTH_MAX], v[_EPST_LENGTH_MAX])
        out = out + v
        out[_EPST_MIN], out[_EPST_MAX], out[_EPST_LENGTH_MAX] = lo, hi, longest
    return out


def reduce_episode_stats(vec: torch.Tensor, world_size: int) -> torch.Tensor:
    """combine_episode_stats over the data-parallel ranks: `vec` [..., EPST SIZE] float64 holds this rank's KBJ_EPST vector(s); returns the
    vector(s) of all ranks' envs together. ONE SUM all-reduce over the counts and sums, ONE MAX all-reduce over (max, -min, longest).
    Collective: every rank calls it, at logging cadence (HumanoidWalkingTask.episode_stats()), never inside the update."""
    if world_size > 1 or FORCE_COLLECTIVE:
        import torch.distributed as dist
        ext = torch.stack([vec[..., _EPST_MAX], -vec[..., _EPST_MIN], vec[..., _EPST_LENGTH_MAX]], dim=-1).contiguous()
        vec = vec.clone()
        vec[..., _EPST_MIN] = 0.0; vec[..., _EPST_MAX] = 0.0       # summed with the rest, overwritten below: keep them finite
        dist.all_reduce(vec, op=dist.ReduceOp.SUM)
        dist.all_reduce(ext, op=dist.ReduceOp.MAX)
        vec[..., _EPST_MAX], vec[..., _EPST_MIN], vec[..., _EPST_LENGTH_MAX] = ext[..., 0], -ext[..., 1], ext[..., 2]
    return vec


# kbj_tracking_stats vectors (kbj_model.h KBJ_TRK_*): every slot is a count or a sum over rows, except the maxima of each mode block
_TRK_MAX = np.zeros(L.TRK["SIZE"], bool)
for _m in range(L.CMODE["COUNT"]):
    _TRK_MAX[_m * L.TRK["MODE_STRIDE"] + L.TRK["MAX"]:_m * L.TRK["MODE_STRIDE"] + L.TRK["MAX"] + L.NTERR] = True


def empty_tracking_stats() -> np.ndarray:
    """The KBJ_TRK vector of no row: zeros (the maxima's identity is 0: the errors are non-negative)."""
    return np.zeros(L.TRK["SIZE"], np.float64)


def combine_tracking_stats(vectors) -> np.ndarray:
    """Statistics of the union of the row sets that the given KBJ_TRK vectors describe (other ranks' envs, or later rollouts): counts and
    sums add up in list order, in float64; the maxima are taken over the list."""
    out = empty_tracking_stats()
    for v in vectors:
        v = np.asarray(v, np.float64)
        out = np.where(_TRK_MAX, np.maximum(out, v), out + v)
    return out


def reduce_tracking_stats(vec: torch.Tensor, world_size: int) -> torch.Tensor:
    """combine_tracking_stats over the data-parallel ranks: `vec` [..., TRK SIZE] float64 holds this rank's KBJ_TRK vector(s); returns the
    vector(s) of all ranks' envs together. ONE SUM all-reduce over the counts and sums, ONE MAX all-reduce over the maxima. Collective:
    every rank calls it, at logging cadence (HumanoidWalkingTask.tracking_stats()), never inside the update."""
    if world_size > 1 or FORCE_COLLECTIVE:
        import torch.distributed as dist
        is_max = torch.from_numpy(_TRK_MAX).to(vec.device)
        hi = torch.where(is_max, vec, torch.zeros_like(vec))
        vec = torch.where(is_max, torch.zeros_like(vec), vec)
        dist.all_reduce(vec, op=dist.ReduceOp.SUM)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        vec = torch.where(is_max, hi, vec)
    return vec
