"""host/dist.py StatsLayout, the slot rule behind the six empty_ / combine_ / reduce_ functions of the episode and tracking statistics: the rule
returns the bytes that the two hand-written combine functions it replaced returned (restated here), and reduce_tracking_stats over two gloo
ranks equals combine_tracking_stats of the ranks' vectors."""
import os

import numpy as np
import torch
import torch.multiprocessing as mp

from kbot_joystick_amd.spec import layout as L
from tests import tracking_ref as TR

E, K, A, M = L.EPST, L.TRK, L.TACC, L.CMODE


def _combine_episode_as_before(vectors):
    """combine_episode_stats as it stood before StatsLayout."""
    lo_i, hi_i, len_i = E["RETURN_MIN"], E["RETURN_MAX"], E["LENGTH_MAX"]
    out = np.zeros(E["SIZE"], np.float64)
    out[lo_i], out[hi_i] = np.inf, -np.inf
    for v in vectors:
        v = np.asarray(v, np.float64)
        lo, hi, longest = min(out[lo_i], v[lo_i]), max(out[hi_i], v[hi_i]), max(out[len_i], v[len_i])
        out = out + v
        out[lo_i], out[hi_i], out[len_i] = lo, hi, longest
    return out


def _trk_max_mask():
    hi = np.zeros(K["SIZE"], bool)
    for m in range(M["COUNT"]):
        hi[m * K["MODE_STRIDE"] + K["MAX"]:m * K["MODE_STRIDE"] + K["MAX"] + L.NTERR] = True
    return hi


def _combine_tracking_as_before(vectors):
    """combine_tracking_stats as it stood before StatsLayout."""
    hi = _trk_max_mask()
    out = np.zeros(K["SIZE"], np.float64)
    for v in vectors:
        v = np.asarray(v, np.float64)
        out = np.where(hi, np.maximum(out, v), out + v)
    return out


def test_combine_returns_the_bytes_of_the_functions_it_replaced():
    """Random float64 vectors of mixed sign and scale (so that the order of the adds shows in the last bit); in the minimum and maximum slots
    every vector holds, by turns, a finite value, +inf or -inf (the tracking maxima, which are non-negative: a finite value or +inf). Lists of
    0 to 4 vectors, the empty vector among them."""
    from kbot_joystick_amd.host import dist as D
    rng = np.random.default_rng(20)
    with np.errstate(invalid="ignore"):            # inf - inf in a slot whose sum is overwritten: both forms add it and both discard it
        for trial in range(200):
            n = int(rng.integers(0, 5))
            ev = [rng.standard_normal(E["SIZE"]) * 10.0 ** rng.integers(-3, 6, E["SIZE"]) for _ in range(n)]
            for v in ev:
                v[E["LENGTH_MAX"]] = abs(v[E["LENGTH_MAX"]])
                for slot in (E["RETURN_MIN"], E["RETURN_MAX"]):
                    v[slot] = rng.choice([v[slot], np.inf, -np.inf])
            tv = [np.abs(rng.standard_normal(K["SIZE"])) * 10.0 ** rng.integers(-3, 6, K["SIZE"]) for _ in range(n)]
            for v in tv:
                hi = _trk_max_mask()
                v[hi] = np.where(rng.random(int(hi.sum())) < 0.2, np.inf, v[hi])
            if n and trial % 3 == 0:
                k = int(rng.integers(0, n))
                ev[k], tv[k] = D.empty_episode_stats(), D.empty_tracking_stats()
            got, want = D.combine_episode_stats(ev), _combine_episode_as_before(ev)
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (trial, got, want)
            got, want = D.combine_tracking_stats(tv), _combine_tracking_as_before(tv)
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (trial, got, want)
    assert D.empty_episode_stats().tobytes() == _combine_episode_as_before([]).tobytes()
    assert D.empty_tracking_stats().tobytes() == np.zeros(K["SIZE"]).tobytes()
    e = D.empty_episode_stats()
    e[0] = 1.0
    assert D.empty_episode_stats()[0] == 0.0                 # a fresh vector every time


def _half(rank):
    """The KBJ_TRK vector of envs [48 rank, 48 rank + 48) of the synthetic problem (8, 96), first call, settle_steps 1."""
    T, N = TR.SHAPES[2]
    aux = TR.problems(T, N).calls[0][:, 48 * rank:48 * rank + 48]
    e32, _ = TR.errors(aux[:T], TR.joint_bias(), TR.STANDARD_HEIGHT, TR.FOOT_ORIGIN_HEIGHT, np.float32)
    return TR.tracking_ref(np.zeros((48, A["SIZE"]), np.float32), e32, aux, 1)[0]


def _reduce_worker(rank, world, port, out):
    import torch.distributed as dist
    from kbot_joystick_amd.host import dist as D
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    mine = _half(rank)
    both = np.stack([mine, D.empty_tracking_stats() if rank else mine])          # a batch of vectors; rank 1's second one is empty
    out[rank] = dict(mine=mine, reduced=D.reduce_tracking_stats(torch.from_numpy(both), world).numpy())
    dist.destroy_process_group()


def test_reduce_tracking_stats_two_ranks_gloo():
    from kbot_joystick_amd.host import dist as D
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_reduce_worker, args=(2, 29557, out), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    hi = _trk_max_mask()
    assert (r0["mine"][hi] > 0).any() and (r1["mine"][hi] > 0).any() and not np.array_equal(r0["mine"], r1["mine"])
    assert r0["reduced"].tobytes() == r1["reduced"].tobytes()
    assert r0["reduced"][0].tobytes() == D.combine_tracking_stats([r0["mine"], r1["mine"]]).tobytes()     # the same arithmetic, in rank order
    assert r0["reduced"][1].tobytes() == r0["mine"].tobytes()
    assert np.array_equal(D.reduce_tracking_stats(torch.from_numpy(r0["mine"]), 1).numpy(), r0["mine"])   # one rank: no collective
