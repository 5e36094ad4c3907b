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


class StatsLayout:
    """The slot rule of a statistics vector that the device builds from partials (kbj_episode_stats, kbj_tracking_stats): every slot is a
    count or a sum, except `max_slots` (maxima, -inf over nothing), `max0_slots` (maxima of non-negative quantities, 0 over nothing) and
    `min_slots` (minima, +inf over nothing). One rule, three uses: the vector of nothing, the union of several vectors on the host, the
    union over the data-parallel ranks."""

    def __init__(self, size: int, max_slots=(), max0_slots=(), min_slots=()):
        self.hi, self.lo = np.array(list(max_slots) + list(max0_slots), np.int64), np.array(list(min_slots), np.int64)
        self._empty = np.zeros(size, np.float64)
        self._empty[list(max_slots)], self._empty[self.lo] = -np.inf, np.inf
        self._ext = np.concatenate([self.hi, self.lo])                                               # what travels through the MAX all-reduce:
        self._sign = np.concatenate([np.ones(len(self.hi)), -np.ones(len(self.lo))])                 # [maxima, -minima]

    def empty(self) -> np.ndarray:
        return self._empty.copy()

    def combine(self, vectors) -> np.ndarray:
        """Statistics of the union of the sets that the given vectors describe (other ranks' envs, or later rollouts): counts and sums add up
        in list order, in float64; maxima and minima are taken over the list. Pure host arithmetic, the same that reduce() performs with
        collectives."""
        out = self.empty()
        for v in vectors:
            v = np.asarray(v, np.float64)
            hi, lo = np.maximum(out[self.hi], v[self.hi]), np.minimum(out[self.lo], v[self.lo])
            out = out + v
            out[self.hi], out[self.lo] = hi, lo
        return out

    def reduce(self, vec: torch.Tensor, world_size: int) -> torch.Tensor:
        """combine() over the data-parallel ranks: `vec` [..., size] float64 holds this rank's vector(s); returns the vector(s) of all ranks'
        envs together. ONE SUM all-reduce over the counts and sums (the other slots zeroed meanwhile: they may be infinite), ONE MAX
        all-reduce over [maxima, -minima]. Collective: every rank calls it, at logging cadence, never inside the update."""
        if world_size > 1 or FORCE_COLLECTIVE:
            import torch.distributed as dist
            slots, sign = torch.from_numpy(self._ext).to(vec.device), torch.from_numpy(self._sign).to(vec.device)
            ext = (vec[..., slots] * sign).contiguous()
            vec = vec.clone()
            vec[..., slots] = 0.0
            dist.all_reduce(vec, op=dist.ReduceOp.SUM)
            dist.all_reduce(ext, op=dist.ReduceOp.MAX)
            vec[..., slots] = ext * sign
        return vec


# kbj_episode_stats vectors (kbj_model.h KBJ_EPST_*): every slot is a count or a sum over the finished episodes, except the extreme returns
# and the longest episode. HumanoidWalkingTask.episode_stats() reduces them
EPISODE_STATS = StatsLayout(L.EPST["SIZE"], max_slots=[L.EPST["RETURN_MAX"]], max0_slots=[L.EPST["LENGTH_MAX"]], min_slots=[L.EPST["RETURN_MIN"]])
empty_episode_stats, combine_episode_stats, reduce_episode_stats = EPISODE_STATS.empty, EPISODE_STATS.combine, EPISODE_STATS.reduce

# kbj_tracking_stats vectors (kbj_model.h KBJ_TRK_*): every slot is a count or a sum over rows, except the maxima of each mode block (the
# errors are non-negative). HumanoidWalkingTask.tracking_stats() reduces them
TRACKING_STATS = StatsLayout(L.TRK["SIZE"], max0_slots=[m * L.TRK["MODE_STRIDE"] + L.TRK["MAX"] + k for m in range(L.CMODE["COUNT"]) for k in range(L.NTERR)])
empty_tracking_stats, combine_tracking_stats, reduce_tracking_stats = TRACKING_STATS.empty, TRACKING_STATS.combine, TRACKING_STATS.reduce

# kbj_gait_stats vectors (kbj_model.h KBJ_GAIT_*, KBJ_GFOOT_*): every slot is a count or a sum, except the largest torque of each mode block and the
# longest swing, longest stance, largest clearance and largest force of each of its foot blocks (all non-negative).
# HumanoidWalkingTask.gait_stats() reduces them
GAIT_STATS = StatsLayout(L.GAIT["SIZE"], max0_slots=[L.gait_slot(m, "TORQUE_MAX") for m in range(L.CMODE["COUNT"])] +
                         [L.gait_slot(m, k, f) for m in range(L.CMODE["COUNT"]) for f in range(2) for k in ("SWING_MAX", "STANCE_MAX", "CLEAR_MAX", "FORCE_MAX")])
empty_gait_stats, combine_gait_stats, reduce_gait_stats = GAIT_STATS.empty, GAIT_STATS.combine, GAIT_STATS.reduce

# kbj_actuator_stats vectors (kbj_model.h KBJ_ACT_*, KBJ_AJNT_*): every slot is a count or a sum, except the largest torque, speed, power and
# action rate of each joint block (all non-negative). HumanoidWalkingTask.actuator_stats() reduces them
ACTUATOR_STATS = StatsLayout(L.ACT["SIZE"], max0_slots=[L.act_slot(m, k, u) for m in range(L.CMODE["COUNT"]) for u in range(L.NU) for k in L.AJNT_MAX])
empty_actuator_stats, combine_actuator_stats, reduce_actuator_stats = ACTUATOR_STATS.empty, ACTUATOR_STATS.combine, ACTUATOR_STATS.reduce
