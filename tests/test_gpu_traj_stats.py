"""kbj_episode_stats and kbj_tracking_stats share one buffer of workgroup partials per context (kbj_traj_stats.hip stats_partials): calls of
both on ONE context, the second needing a larger buffer than the first left, return the bytes each call returns alone on a fresh context."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import tracking_ref as TR
from tests.test_gpu_episode_stats import UZ, _problem

pytestmark = pytest.mark.gpu
E, EA, K, A, R = L.EPST, L.EACC, L.TRK, L.TACC, L.TERR


def _context():
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.spec import compiler
    return B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=64, batch_size=64, hidden_size=64, rollout_len=8, unhealthy_z=UZ))


def _tracking(ctx, aux, acc0):
    """One kbj_tracking_stats call (settle_steps 2, with err_d) on aux [T + 1, N, AUX SIZE] from the carry rows acc0 -> (acc, stats, err) as numpy."""
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    T, N = aux.shape[0] - 1, aux.shape[1]
    traj = TrajBuffers(T, N, 64, 2, dev)
    traj.aux.copy_(torch.from_numpy(aux))
    acc = torch.from_numpy(acc0.copy()).to(dev)
    stats = torch.full((K["SIZE"],), -1.0, dtype=torch.float64, device=dev)
    err = torch.full((T, N, R["SIZE"]), -1.0, device=dev)
    ctx.tracking_stats(traj.c, 2, acc, stats, err)
    return acc.cpu().numpy(), stats.cpu().numpy(), err.cpu().numpy()


def _episode(ctx, reward, aux, comps):
    """One kbj_episode_stats call with reward terms, from fresh accumulator rows -> (acc, stats) as numpy."""
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    T, N = reward.shape
    traj = TrajBuffers(T, N, 64, 2, dev, reward_comps=True)
    traj.reward.copy_(torch.from_numpy(reward)); traj.aux.copy_(torch.from_numpy(aux)); traj.comps.copy_(torch.from_numpy(comps))
    acc = torch.zeros(N, EA["SIZE"], device=dev)
    stats = torch.full((E["SIZE"],), -1.0, dtype=torch.float64, device=dev)
    ctx.episode_stats(traj.c, acc, stats)
    return acc.cpu().numpy(), stats.cpu().numpy()


def test_one_partial_buffer_serves_both_statistics_in_turn():
    """On ONE context, in this order:
      kbj_tracking_stats at T = 7, N = 64: one workgroup, a 6-step chunk and one step; the first call allocates the buffer, 128 doubles;
      kbj_episode_stats at T = 9, N = 130: three workgroups, an 8-step chunk and one step; 3 x 32 doubles over the tracking partials;
      kbj_tracking_stats at T = 7, N = 64 again (the problem's second call, from the first call's carry rows) over the episode partials;
      kbj_episode_stats at T = 9, N = 321: six workgroups, 192 doubles - the capacity is counted in doubles, so this is the call that grows it.
    Each call's acc, stats and (tracking) err have the bytes of the same call made alone on a fresh context."""
    trk = TR.problems(7, 64).calls
    fresh = np.zeros((64, A["SIZE"]), np.float32)
    ep130, ep321 = _problem(np.random.default_rng(9130), 9, 130), _problem(np.random.default_rng(9321), 9, 321)

    def alone(call, *args):
        ctx = _context()
        try:
            return call(ctx, *args)
        finally:
            ctx.close()

    want = [alone(_tracking, trk[0], fresh), alone(_episode, *ep130)]
    want += [alone(_tracking, trk[1], want[0][0]), alone(_episode, *ep321)]
    assert want[0][1][K["EPISODES"]] >= 64 and want[2][1][K["EPISODES"]] > 0 and want[1][1][E["EPISODES"]] > 130 and want[3][1][E["EPISODES"]] > 321     # the calls have something to say
    assert want[0][1].tobytes() != want[2][1].tobytes()
    ctx = _context()
    try:
        got = [_tracking(ctx, trk[0], fresh), _episode(ctx, *ep130)]
        got += [_tracking(ctx, trk[1], got[0][0]), _episode(ctx, *ep321)]
    finally:
        ctx.close()
    for name, g3, w3 in zip(("tracking", "episode", "tracking again", "episode, wider"), got, want):
        for part, g, w in zip(("acc", "stats", "err"), g3, w3):
            assert g.tobytes() == w.tobytes(), f"{name}: {part} differs from the same call alone on a fresh context"
