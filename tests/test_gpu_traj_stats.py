"""kbj_episode_stats and kbj_tracking_stats share one buffer of workgroup partials per context (kbj_traj_stats.hip stats_partials): calls of
both on ONE context, the second needing a larger buffer than the first left, return the bytes each call returns alone on a fresh context.
kbj_push_recovery and kbj_step_response share the staging of their group reduce (kbj_window_scan.h), 256 envs a round: both at N = 257 and
N = 513, a second round of one env and a third, against their restatements."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import push_ref as PR, step_response_ref as SR, tracking_ref as TR
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


@pytest.fixture(scope="module")
def gctx():
    ctx = _context()
    yield ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


GROUPINGS = [(1, True), (3, True), (256, True), (1, False)]     # (G, with group_d); group_d = NULL: every env in group 0


@pytest.mark.parametrize("N", [257, 513])
def test_push_recovery_group_reduce_over_several_rounds(gctx, N):
    """T = 24, N = 257 and 513: the record rows equal recovery_ref bit for bit; for G in (1, 3, 256), and for group_d = NULL with G = 1,
    the statistics equal group_stats_ref of the device's records as uint64."""
    import torch
    from kbot_joystick_amd.host import binding as B
    T, dev = 24, torch.device("cuda", 0)
    prob = PR.problems(T, N)
    want_rec, _ = PR.recovery_ref(prob.err, prob.done, prob.sched, prob.tol, prob.hold, prob.window)
    aux, err, sched = torch.from_numpy(prob.aux).to(dev), torch.from_numpy(prob.err).to(dev), torch.from_numpy(prob.sched).to(dev)
    crit = B.PushCriteria((B.C.c_float * L.NTERR)(*prob.tol), prob.hold, prob.window)
    for G, grouped in GROUPINGS:
        group = PR.groups(N, G) if grouped else None
        rec = torch.full((N, L.PREC["SIZE"]), -7.0, device=dev)
        stats = torch.full((G, L.PSTAT["SIZE"]), -7.0, dtype=torch.float64, device=dev)
        gctx.push_recovery(B.Traj(T=T, N=N, aux_d=aux.data_ptr()), err, sched, crit, rec, None if group is None else torch.from_numpy(group).to(dev), G, stats)
        gctx.synchronize()
        rec, stats = rec.cpu().numpy(), stats.cpu().numpy()
        assert np.array_equal(_bits(rec), _bits(want_rec)), np.argwhere(_bits(rec) != _bits(want_rec))[:5]
        want = PR.group_stats_ref(rec, group, G)
        assert np.array_equal(stats.view(np.uint64), want.view(np.uint64)), (G, grouped, np.argwhere(stats.view(np.uint64) != want.view(np.uint64))[:8])


@pytest.mark.parametrize("hold", [1, 4])
@pytest.mark.parametrize("N", [257, 513])
def test_step_response_group_reduce_over_several_rounds(gctx, N, hold):
    """T = 75, N = 257 and 513, hold 1 and 4, smoothing over 3 rows: the records equal scan_ref on the device's own signal bit for bit; for
    G in (1, 3, 256), and for group_d = NULL with G = 1, the statistics equal group_stats_ref of the device's records as uint64."""
    import torch
    from kbot_joystick_amd.host import binding as B
    T, dev = 75, torch.device("cuda", 0)
    prob = SR.problem(hold, T, N)
    c = SR.criteria(3, hold)
    f3 = B.C.c_float * L.NSCH
    crit = B.StepCriteria(f3(*c.min_step), f3(*c.band_abs), c.band_frac, c.rise_level, c.smooth, c.hold, c.window)
    aux, sched = torch.from_numpy(prob.aux).to(dev), torch.from_numpy(prob.sched).to(dev)
    for G, grouped in GROUPINGS:
        group = SR.groups(N, G) if grouped else None
        sig = torch.full((T, N, L.SSIG["SIZE"]), -7.0, device=dev)
        rec = torch.full((N, L.SREC["SIZE"]), -7.0, device=dev)
        stats = torch.full((G, L.SSTAT["SIZE"]), -7.0, dtype=torch.float64, device=dev)
        gctx.step_response(B.Traj(T=T, N=N, aux_d=aux.data_ptr()), sched, crit, sig, rec, None if group is None else torch.from_numpy(group).to(dev), G, stats)
        gctx.synchronize()
        sig, rec, stats = sig.cpu().numpy(), rec.cpu().numpy(), stats.cpu().numpy()
        want_rec, _ = SR.scan_ref(sig, prob.sched, c)                      # on the device's own signal
        assert np.array_equal(_bits(rec), _bits(want_rec)), np.argwhere(_bits(rec) != _bits(want_rec))[:8]
        want = SR.group_stats_ref(rec, group, G)
        assert np.array_equal(stats.view(np.uint64), want.view(np.uint64)), (G, grouped, np.argwhere(stats.view(np.uint64) != want.view(np.uint64))[:8])
