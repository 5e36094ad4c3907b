"""kbj_actuator_stats on the GPU: the synthetic problems of tests/actuator_ref.py through the C ABI against the host restatement, one real
rollout, bit-reproducibility and the argument checks.

Bounds. The carry rows, the per-env record, every count and every maximum: exact - they are whole numbers below 2^53 or fp32 maxima, and the
per-env sums are float64 sums in a stated order rounded once. The double sums of real values (TAU_SQ, VEL_SQ, POW_ABS, POW_POS, DACT_SQ,
SPEED_SUM): within 1e-9 * sum |x_i| of math.fsum - double accumulation of at most ~2,000 values errs by at most count * 2^-53 * sum |x|
~ 2e-13 * sum |x| whatever the reduction tree; the margin is derived in tests/test_gpu_episode_stats.py, not measured."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import actuator_ref as AR

pytestmark = pytest.mark.gpu
V, J, A, E, X, M = L.ACT, L.AJNT, L.AACC, L.AENV, L.AUX, L.CMODE
NU = L.NU
SCAN, REDUCE = "kbj::actuator_stats_kernel", "kbj::ordered_reduce_wide_kernel<kbj::ActSlots>"


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


def _count(vec, k):
    return int(sum(vec[L.act_slot(m, k, u)] for m in range(M["COUNT"]) for u in range(NU)))


@pytest.mark.parametrize("T,N", AR.SHAPES)
def test_synthetic_trajectories_match_the_restatement(ctx, T, N):
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    P, ref = AR.problems(T, N), AR.reference(T, N)
    lv = AR.c_levels(P.lv)
    traj = TrajBuffers(T, N, 64, 2, dev, record_state=True)
    acc = torch.from_numpy(P.acc0.copy()).to(dev)                                  # the spare floats hold 7.0
    for call, (aux, qs, act) in enumerate(P.calls):
        before, after, want, mags, env_want = ref[call]
        traj.aux.copy_(torch.from_numpy(aux)); traj.qstate.copy_(torch.from_numpy(qs)); traj.action.copy_(torch.from_numpy(act))
        stats = torch.full((V["SIZE"],), -1.0, dtype=torch.float64, device=dev)     # overwritten, spare slots included
        env = torch.full((N, E["SIZE"]), -1.0, device=dev)
        start = acc.clone()
        assert start.cpu().numpy().tobytes() == before.tobytes()
        ctx.actuator_stats(traj.c, lv, acc, stats, env)
        got, a, e = stats.cpu().numpy(), acc.cpu().numpy(), env.cpu().numpy()
        assert np.array_equal(_bits(a), _bits(after)), ("carry rows differ from the restatement", np.argwhere(_bits(a) != _bits(after))[:8])
        assert (a[:, A["RUNNING"] + 1:] == 7.0).all()
        assert np.array_equal(_bits(e), _bits(env_want)), ("per-env records differ from the restatement", np.argwhere(_bits(e) != _bits(env_want))[:8], e[:2], env_want[:2])
        AR.assert_stats_match(got, want, mags)
        # the same inputs without env_d: the same bytes; and once more with it: the same bytes again
        for with_env in (False, True):
            acc2, stats2 = start.clone(), torch.zeros(V["SIZE"], dtype=torch.float64, device=dev)
            env2 = torch.zeros(N, E["SIZE"], device=dev) if with_env else None
            ctx.actuator_stats(traj.c, lv, acc2, stats2, env2)
            assert acc2.cpu().numpy().tobytes() == a.tobytes() and stats2.cpu().numpy().tobytes() == got.tobytes()
            assert env2 is None or env2.cpu().numpy().tobytes() == e.tobytes()
        print(f"T={T} N={N} call {call}: {int(got[V['EPISODES']])} episodes, {_count(got, 'TAU_ROWS')} / {_count(got, 'VEL_ROWS')} / {_count(got, 'STOP_ROWS')} "
              f"(row, joint) pairs at the torque level / over speed / at a stop of {T * N * NU}")


def test_refusals_launch_nothing_and_a_good_call_launches_two_kernels(ctx):
    import ctypes
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    traj = TrajBuffers(2, 4, 64, 2, dev, record_state=True)
    acc, stats = torch.full((4, A["SIZE"]), 3.0, device=dev), torch.full((V["SIZE"],), -1.0, dtype=torch.float64, device=dev)
    env = torch.zeros(4 * E["SIZE"] + 4, device=dev)
    lv = AR.c_levels(AR.synthetic_levels())
    lib = B.load_library()

    def variant(**kw):          # the trajectory with one member changed
        t = B.Traj.from_buffer_copy(traj.c)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def levels(name, u, value):  # the levels with one entry changed
        out = B.ActuatorLevels.from_buffer_copy(lv)
        getattr(out, name)[u] = value
        return out
    ctx.profile_begin()
    for args in ((traj.c, lv, None, stats), (traj.c, lv, acc, None), (traj.c, None, acc, stats), (None, lv, acc, stats)):
        with pytest.raises(B.KbjError, match="null argument"):
            ctx.actuator_stats(*args)
    assert lib.kbj_actuator_stats(None, ctypes.byref(traj.c), ctypes.byref(lv), acc.data_ptr(), stats.data_ptr(), None) != 0 and b"null argument" in lib.kbj_last_error(None)
    with pytest.raises(B.KbjError, match="no qstate_d.*record_state"):
        ctx.actuator_stats(variant(qstate_d=None), lv, acc, stats)
    for t in (variant(aux_d=None), variant(action_d=None), variant(T=0), variant(N=-1)):
        with pytest.raises(B.KbjError, match="needs aux_d, action_d, qstate_d and positive T, N"):
            ctx.actuator_stats(t, lv, acc, stats)
    for args in ((traj.c, lv, acc.data_ptr() + 4, stats), (traj.c, lv, acc, stats, env.data_ptr() + 4), (variant(aux_d=traj.aux.data_ptr() + 8), lv, acc, stats),
                 (variant(qstate_d=traj.qstate.data_ptr() + 4), lv, acc, stats), (variant(action_d=traj.action.data_ptr() + 8), lv, acc, stats)):
        with pytest.raises(B.KbjError, match="16-byte aligned"):
            ctx.actuator_stats(*args)
    nan, inf = float("nan"), float("inf")
    for bad, what in ((levels("tau_level", 7, nan), "tau_level"), (levels("tau_level", 0, 0.0), "tau_level"), (levels("tau_level", 19, -1.0), "tau_level"),
                      (levels("vel_level", 3, nan), "vel_level"), (levels("vel_level", 4, 0.0), "vel_level"), (levels("pos_lo", 5, nan), "pos_lo"),
                      (levels("pos_hi", 6, nan), "pos_lo"), (levels("pos_lo", 8, 5.0), "pos_lo > pos_hi")):
        with pytest.raises(B.KbjError, match=what):
            ctx.actuator_stats(traj.c, bad, acc, stats)
    names = [k["name"] for k in ctx.profile_end()["kernels"]]
    assert not any("actuator" in n or "ActSlots" in n for n in names), names
    assert (stats.cpu().numpy() == -1).all() and (acc.cpu().numpy() == 3.0).all()
    # a good call: the scan and the wide reduce, once each; +inf speed levels and pos_lo == pos_hi are accepted
    acc.zero_()
    ok = levels("pos_lo", 9, float(lv.pos_hi[9]))
    ok.vel_level[0] = inf
    ctx.profile_begin()
    ctx.actuator_stats(traj.c, ok, acc, stats, env[:4 * E["SIZE"]])
    kernels = {k["name"]: k["launches"] for k in ctx.profile_end()["kernels"]}
    assert kernels == {SCAN: 1, REDUCE: 1}, kernels
    got = stats.cpu().numpy()
    # zero rows: eight standing rows, four episode starts, four pairs, nothing at a level - but joint 9, whose band is one point: always at its stop
    S = M["STAND"]
    assert got[L.act_slot(S, "ROWS")] == 8 and got[L.act_slot(S, "PAIRS")] == 4 and got[V["EPISODES"]] == 4
    assert got[L.act_slot(S, "STOP_ROWS", 9)] == 8 and got[L.act_slot(S, "ANY_STOP_ROWS")] == 8 and got.sum() == 32
    e = env[:4 * E["SIZE"]].cpu().numpy().reshape(4, E["SIZE"])
    assert (e[:, E["ROWS"]] == 2).all() and (e[:, E["PAIRS"]] == 1).all() and (e[:, E["ANY_STOP_ROWS"]] == 2).all() and (e[:, E["PEAK_JOINT"]] == 0).all() and e.sum() == 20


def test_a_real_rollout_matches_the_restatement():
    """kbj_rollout of 64 envs x 24 steps with the state record, with the parameters kbj_init_params draws, on kbot-headless: the kernel on its
    rows equals the restatement on the same rows, with the robot's own levels (host/actuator.actuator_levels) and with a speed limit. How
    many rows hit a level under a fresh policy is printed, not asserted."""
    import torch
    from kbot_joystick_amd.host import actuator as HA, binding as B
    from kbot_joystick_amd.host.buffers import CarryBuffers, TrajBuffers
    from kbot_joystick_amd.spec import compiler
    dev = torch.device("cuda", 0)
    T, N = 24, 64
    model = compiler.load_model("kbot-headless")
    c = B.Context(model, L.default_config(num_envs=N, batch_size=N, hidden_size=64, rollout_len=T))
    try:
        params = torch.zeros(c.param_count(), device=dev)
        c.init_params(5, params)
        traj, carry = TrajBuffers(T, N, 64, 2, dev, record_state=True), CarryBuffers(N, 64, 2, dev)
        c.env_reset_all(5, traj.actor_obs[T], traj.critic_obs[T], traj.aux[T])
        lv = HA.actuator_levels(model, torque_level=0.5, speed_limit=4.0)
        lvd = AR.levels_dict(lv)
        acc, acc_ref = torch.zeros(N, A["SIZE"], device=dev), np.zeros((N, A["SIZE"]), np.float32)
        for it in range(2):
            c.rollout(params, carry.c, 5, it * T, traj.c)
            stats, env = torch.zeros(V["SIZE"], dtype=torch.float64, device=dev), torch.zeros(N, E["SIZE"], device=dev)
            c.actuator_stats(traj.c, lv, acc, stats, env)
            got = stats.cpu().numpy()
            want, mags, env_want = AR.actuator_ref(acc_ref, traj.aux.cpu().numpy(), traj.qstate.cpu().numpy(), traj.action.cpu().numpy(), T, lvd)
            assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc_ref)) and np.array_equal(_bits(env.cpu().numpy()), _bits(env_want))
            AR.assert_stats_match(got, want, mags)
            rows = sum(got[L.act_slot(m, "ROWS")] for m in range(M["COUNT"]))
            assert rows == T * N and got[L.act_slot(0, "TAU_SQ", 3)] + got[L.act_slot(5, "TAU_SQ", 3)] > 0
            any_tau, any_stop = (int(sum(got[L.act_slot(m, k)] for m in range(M["COUNT"]))) for k in ("ANY_TAU_ROWS", "ANY_STOP_ROWS"))
            print(f"rollout {it}: {int(got[V['EPISODES']])} episode starts; of {T * N} rows {any_tau} have a joint at half its torque limit, {any_stop} a joint at a stop; "
                  f"of {T * N * NU} (row, joint) pairs {_count(got, 'TAU_ROWS')} at the torque level, {_count(got, 'VEL_ROWS')} over 4 rad/s, {_count(got, 'STOP_ROWS')} at a stop")
    finally:
        c.close()
