"""kbj_gait_stats on the GPU: the synthetic problems of tests/gait_ref.py through the C ABI against the host restatement, one real rollout,
bit-reproducibility and the argument checks.

Bounds. The carry rows, the per-env record, every count, duration sum, sum of squares and maximum: exact - they are whole numbers below 2^53
or fp32 maxima, and the per-env sums are float64 sums in row order rounded once. The double sums of real values (CLEAR_SUM, CLEAR_SUMSQ,
FORCE_SUM, TORQUE_SQ): within 1e-9 * sum |x_i| of math.fsum - double accumulation of at most ~2,000 values errs by at most
count * 2^-53 * sum |x| ~ 2e-13 * sum |x| whatever the reduction tree; the margin is derived in tests/test_gpu_episode_stats.py, not measured."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import gait_ref as GR

pytestmark = pytest.mark.gpu
G, F, A, E, X, M = L.GAIT, L.GFOOT, L.GACC, L.GENV, L.AUX, L.CMODE


def _context(n):
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.spec import compiler
    return B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=n, batch_size=n, hidden_size=64, rollout_len=8))


@pytest.fixture(scope="module")
def ctx():
    c = _context(64)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("T,N", GR.SHAPES)
def test_synthetic_trajectories_match_the_restatement(ctx, T, N):
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    P, ref = GR.problems(T, N), GR.reference(T, N)
    traj = TrajBuffers(T, N, 64, 2, dev)
    acc = torch.from_numpy(P.acc0.copy()).to(dev)                                  # the spare floats hold 7.0
    for call, aux in enumerate(P.calls):
        before, after, want, mags, env_want, _ = ref[call]
        traj.aux.copy_(torch.from_numpy(aux))
        stats = torch.full((G["SIZE"],), -1.0, dtype=torch.float64, device=dev)     # overwritten, spare slots included
        env = torch.full((N, E["SIZE"]), -1.0, device=dev)
        start = acc.clone()
        assert start.cpu().numpy().tobytes() == before.tobytes()
        ctx.gait_stats(traj.c, acc, stats, env)
        got, a, e = stats.cpu().numpy(), acc.cpu().numpy(), env.cpu().numpy()
        assert np.array_equal(_bits(a), _bits(after)), ("carry rows differ from the restatement", np.argwhere(_bits(a) != _bits(after))[:8])
        assert (a[:, [5, 11, 14, 15]] == 7.0).all()
        assert np.array_equal(_bits(e), _bits(env_want)), ("per-env records differ from the restatement", np.argwhere(_bits(e) != _bits(env_want))[:8])
        GR.assert_stats_match(got, want, mags)
        # the same inputs without env_d: the same bytes; and once more with it: the same bytes again
        for with_env in (False, True):
            acc2, stats2 = start.clone(), torch.zeros(G["SIZE"], dtype=torch.float64, device=dev)
            env2 = torch.zeros(N, E["SIZE"], device=dev) if with_env else None
            ctx.gait_stats(traj.c, acc2, stats2, env2)
            assert acc2.cpu().numpy().tobytes() == a.tobytes() and stats2.cpu().numpy().tobytes() == got.tobytes()
            assert env2 is None or env2.cpu().numpy().tobytes() == e.tobytes()
        events = sum(got[L.gait_slot(m, k, f)] for m in range(M["COUNT"]) for f in range(2) for k in ("TOUCHDOWNS", "LIFTOFFS"))
        print(f"T={T} N={N} call {call}: {int(got[G['EPISODES']])} episodes, {int(events)} events")


def test_null_and_misaligned_arguments_fail_and_launch_nothing(ctx):
    import ctypes
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    traj = TrajBuffers(2, 4, 64, 2, dev)
    acc, stats = torch.full((4, A["SIZE"]), 3.0, device=dev), torch.full((G["SIZE"],), -1.0, dtype=torch.float64, device=dev)
    env = torch.zeros(4 * E["SIZE"] + 4, device=dev)
    lib = B.load_library()

    def variant(**kw):          # the trajectory with one member changed
        t = B.Traj.from_buffer_copy(traj.c)
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    ctx.profile_begin()
    for args in ((traj.c, None, stats), (traj.c, acc, None)):
        with pytest.raises(B.KbjError, match="null argument"):
            ctx.gait_stats(*args)
    assert lib.kbj_gait_stats(ctx._h, None, acc.data_ptr(), stats.data_ptr(), None) != 0 and b"null argument" in lib.kbj_last_error(ctx._h)
    assert lib.kbj_gait_stats(None, ctypes.byref(traj.c), acc.data_ptr(), stats.data_ptr(), None) != 0 and b"null argument" in lib.kbj_last_error(None)
    for t in (variant(aux_d=None), variant(T=0), variant(N=0)):
        with pytest.raises(B.KbjError, match="needs aux_d and positive T, N"):
            ctx.gait_stats(t, acc, stats)
    for args in ((traj.c, acc.data_ptr() + 4, stats), (traj.c, acc, stats, env.data_ptr() + 4), (variant(aux_d=traj.aux.data_ptr() + 8), acc, stats)):
        with pytest.raises(B.KbjError, match="16-byte aligned"):
            ctx.gait_stats(*args)
    names = [k["name"] for k in ctx.profile_end()["kernels"]]
    assert not any("gait_stats" in n for n in names), names
    assert (stats.cpu().numpy() == -1).all() and (acc.cpu().numpy() == 3.0).all()
    acc.zero_()
    ctx.profile_begin()
    ctx.gait_stats(traj.c, acc, stats, env[:4 * E["SIZE"]])
    kernels = {k["name"]: k["launches"] for k in ctx.profile_end()["kernels"]}
    assert kernels == {"kbj::gait_stats_kernel": 1}
    got = stats.cpu().numpy()
    assert got[L.gait_slot(M["STAND"], "ROWS")] == 8 and got[L.gait_slot(M["STAND"], "FLIGHT")] == 8 and got[G["EPISODES"]] == 4 and got.sum() == 20      # zero rows: eight standing rows in the air


def test_a_real_rollout_matches_the_restatement():
    """kbj_rollout of 64 envs x 24 steps with the parameters kbj_init_params draws, on kbot-headless: the kernel on its aux rows equals the
    restatement on the same rows. How many events a fresh policy produces is printed, not asserted."""
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.buffers import CarryBuffers, TrajBuffers
    from kbot_joystick_amd.spec import compiler
    dev = torch.device("cuda", 0)
    T, N = 24, 64
    c = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=N, batch_size=N, hidden_size=64, rollout_len=T))
    try:
        params = torch.zeros(c.param_count(), device=dev)
        c.init_params(5, params)
        traj, carry = TrajBuffers(T, N, 64, 2, dev), CarryBuffers(N, 64, 2, dev)
        c.env_reset_all(5, traj.actor_obs[T], traj.critic_obs[T], traj.aux[T])
        acc, acc_ref = torch.zeros(N, A["SIZE"], device=dev), np.zeros((N, A["SIZE"]), np.float32)
        for it in range(2):
            c.rollout(params, carry.c, 5, it * T, traj.c)
            stats, env = torch.zeros(G["SIZE"], dtype=torch.float64, device=dev), torch.zeros(N, E["SIZE"], device=dev)
            c.gait_stats(traj.c, acc, stats, env)
            got, aux = stats.cpu().numpy(), traj.aux.cpu().numpy()
            want, mags, env_want, _ = GR.gait_ref(acc_ref, aux, T)
            assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc_ref)) and np.array_equal(_bits(env.cpu().numpy()), _bits(env_want))
            GR.assert_stats_match(got, want, mags)
            rows = sum(got[L.gait_slot(m, "ROWS")] for m in range(M["COUNT"]))
            assert rows == T * N
            count = lambda k: int(sum(got[L.gait_slot(m, k, f)] for m in range(M["COUNT"]) for f in range(2)))
            print(f"rollout {it}: {int(got[G['EPISODES']])} episode starts, {count('TOUCHDOWNS')} touchdowns, {count('LIFTOFFS')} lift-offs, {count('SWING_N')} counted swings, "
                  f"{count('STANCE_N')} counted stances, {int(sum(got[L.gait_slot(m, 'FLIGHT')] for m in range(M['COUNT'])))} flight rows, "
                  f"{int(sum(got[L.gait_slot(m, 'REPEATS')] for m in range(M['COUNT'])))} repeats")
    finally:
        c.close()
