"""kbj_tracking_stats on the GPU: the synthetic problems of tests/tracking_ref.py through the C ABI against the host restatement, the link to
rewards_kernel, bit-reproducibility and the argument checks.

Bounds. Mode, settled flag, since, the carry rows, every count and every maximum (against the kernel's own fp32 err_d rows): exact. Every
double sum: within 1e-9 * sum |x_i| of math.fsum over the err_d rows - double accumulation of at most ~2,000 fp32 values errs by at most
count * 2^-53 * sum |x| ~ 2e-13 * sum |x| whatever the reduction tree; the margin is not a measured tolerance (tests/test_gpu_episode_stats.py).
The five error columns against the float64 reference: max(4 S_k, 8 * 2^-24 M_k), S_k = the float32 restatement's own distance from float64
over the issue's problems, M_k the largest operand magnitude (tracking_ref.error_bounds; tests/test_tracking_host.py prints them; the two
chunk-boundary shapes added here come from the same generator and are held to the same figures). The reward
terms against exp(-f(err) / scale) formed in float64 from the err_d row: that bound / scale + 4 * 2^-24, since |d exp(-x)| <= |dx| (for the
walking branch of linvel, f = err^2: |d exp(-e^2 / s)| = (2 e / s) exp(-e^2 / s) |de| <= 0.86 / sqrt(s) |de| < |de| / s at s = 0.2).
Measured worst errors / bounds on an MI355X: EXPERIMENTS.md "Tracking errors"."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import constants, layout as L
from tests import tracking_ref as TR

pytestmark = pytest.mark.gpu
K, A, R, X = L.TRK, L.TACC, L.TERR, L.AUX
NE = L.NTERR


def _context(n):
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.spec import compiler
    return B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=n, batch_size=n, hidden_size=64, rollout_len=8))


@pytest.fixture(scope="module")
def ctx():
    c = _context(64)
    assert (c.config.rew_standard_height, c.config.rew_foot_origin_height) == (np.float32(TR.STANDARD_HEIGHT), np.float32(TR.FOOT_ORIGIN_HEIGHT))
    assert np.array_equal(np.array(c.model.joint_bias, np.float32), TR.joint_bias())
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# Beside the issue's shapes, the chunking of the kernel (6 time steps per chunk, results and last commands double-buffered by chunk parity):
# T an exact multiple of the chunk with three chunks, so that the last staging wavefront owns row T - 1 and a buffer is used a second time;
# and four chunks with a one-step tail.
CHUNK_SHAPES = [(18, 65), (19, 70)]


@pytest.mark.parametrize("T,N", TR.SHAPES + CHUNK_SHAPES)
def test_synthetic_trajectories_match_the_restatement(ctx, T, N):
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    bounds = TR.error_bounds()
    e64 = [TR.errors(aux[:T], TR.joint_bias(), TR.STANDARD_HEIGHT, TR.FOOT_ORIGIN_HEIGHT, np.float64)[0] for aux in TR.problems(T, N).calls]
    traj = TrajBuffers(T, N, 64, 2, dev)
    worst = np.zeros(NE)
    for settle in (0, 3, T + 1):
        acc_ref = np.zeros((N, A["SIZE"]), np.float32)
        acc_ref[:, A["RUNNING"] + 1:] = 7.0                                  # the spare floats of a row are left alone
        acc = torch.from_numpy(acc_ref.copy()).to(dev)
        seen = np.zeros(K["SIZE"])
        for call, aux in enumerate(TR.problems(T, N).calls):
            traj.aux.copy_(torch.from_numpy(aux))
            stats = torch.full((K["SIZE"],), -1.0, dtype=torch.float64, device=dev)       # overwritten, spare slots included
            err = torch.full((T, N, R["SIZE"]), -1.0, device=dev)
            start = acc.clone()
            ctx.tracking_stats(traj.c, settle, acc, stats, err)
            got, e = stats.cpu().numpy(), err.cpu().numpy()
            want, mags, rows = TR.tracking_ref(acc_ref, e, aux, settle)       # the statistics of the kernel's own fp32 rows
            assert np.array_equal(e[:, :, R["MODE"]], rows[:, :, 0]) and np.array_equal(e[:, :, R["SETTLED"]], rows[:, :, 1]) and np.array_equal(e[:, :, R["SINCE"]], rows[:, :, 2])
            assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc_ref)), "carry rows differ from the restatement"
            TR.assert_stats_match(got, want, mags)
            d = np.abs(e[:, :, :NE].astype(np.float64) - e64[call]).reshape(-1, NE).max(0)
            worst = np.maximum(worst, d)
            assert (d <= bounds).all(), (d, bounds)
            # the same inputs without err_d: the same bytes
            acc2, stats2 = start.clone(), torch.zeros(K["SIZE"], dtype=torch.float64, device=dev)
            ctx.tracking_stats(traj.c, settle, acc2, stats2, None)
            assert acc2.cpu().numpy().tobytes() == acc.cpu().numpy().tobytes() and stats2.cpu().numpy().tobytes() == got.tobytes()
            seen += got
        assert seen[K["EPISODES"]] >= N                                      # a fresh carry: every env starts an episode on row 0 of the first call
        if settle == T + 1 and N >= 4:                                        # only a command held across a call boundary gets there: env 1's
            assert sum(seen[m * K["MODE_STRIDE"] + K["SETTLED"]] for m in range(L.CMODE["COUNT"])) >= 2 * T - 1
        if settle == 0:
            assert all(seen[m * K["MODE_STRIDE"] + K["SETTLED"]] == seen[m * K["MODE_STRIDE"] + K["ROWS"]] for m in range(L.CMODE["COUNT"]))
    for k, name in enumerate(constants.TRACKING_ERROR_NAMES):
        print(f"T={T} N={N} {name}: worst |err_d - float64| {worst[k]:.3e} (bound {bounds[k]:.3e})")


def test_reward_terms_follow_from_the_error_rows():
    """The same aux rows through kbj_rewards with reward_comps: the five tracking terms equal exp(-f(err) / scale) of the err_d row."""
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    T, N = TR.SHAPES[2]
    c = _context(N)
    cfg, bounds = c.config, TR.error_bounds()
    traj = TrajBuffers(T, N, 64, 2, dev, reward_comps=True)
    c.env_reset_all(0, traj.actor_obs[T], traj.critic_obs[T], traj.aux[T])     # initialises the reward carries
    aux = TR.problems(T, N).calls[0]
    traj.aux.copy_(torch.from_numpy(aux))
    err = torch.zeros(T, N, R["SIZE"], device=dev)
    c.tracking_stats(traj.c, 0, torch.zeros(N, A["SIZE"], device=dev), torch.zeros(K["SIZE"], dtype=torch.float64, device=dev), err)
    c.rewards(traj.aux, T, traj.reward, traj.comps)
    e, comps = err.cpu().numpy().astype(np.float64), traj.comps.cpu().numpy().astype(np.float64)
    c.close()
    cmd = aux[:T, :, X["CMD"]:X["CMD"] + 3].astype(np.float64)
    zc = np.sqrt((cmd * cmd).sum(-1)) < 1e-3
    assert zc.any() and (~zc).any()
    lin = e[:, :, R["LIN"]]
    terms = (("LINVEL", R["LIN"], np.where(zc, lin, lin * lin), cfg.rew_linvel_err), ("ANGVEL", R["YAW"], e[:, :, R["YAW"]], cfg.rew_angvel_err),
             ("ROLL_PITCH", R["TILT"], e[:, :, R["TILT"]], np.where(zc, cfg.rew_rollpitch_err_zero, cfg.rew_rollpitch_err)),
             ("BASE_HEIGHT", R["HEIGHT"], e[:, :, R["HEIGHT"]], cfg.rew_height_err), ("ARM_POS", R["ARM"], e[:, :, R["ARM"]], cfg.rew_armpos_err))
    for k, (name, col, f, scale) in enumerate(terms):
        scale = np.asarray(scale, np.float64)
        d = np.abs(comps[:, :, k] - np.exp(-f / scale))
        bound = bounds[col] / scale + 4 * 2.0 ** -24
        print(f"{name}: worst |comps - exp(-f(err_d) / scale)| {d.max():.3e} (bound {np.max(bound):.3e})")
        assert constants.REWARD_NAMES[k] == name.lower() and (d <= bound).all(), (name, d.max())


def test_null_and_misaligned_arguments_fail_and_launch_nothing(ctx):
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    traj = TrajBuffers(2, 4, 64, 2, dev)
    acc, stats = torch.zeros(4, A["SIZE"], device=dev), torch.full((K["SIZE"],), -1.0, dtype=torch.float64, device=dev)
    err = torch.zeros(2 * 4 * R["SIZE"] + 4, device=dev)
    ctx.profile_begin()
    for args in ((traj.c, 0, None, stats), (traj.c, 0, acc, None)):
        with pytest.raises(B.KbjError, match="null argument"):
            ctx.tracking_stats(*args)
    for args in ((traj.c, 0, acc.data_ptr() + 4, stats), (traj.c, 0, acc, stats, err.data_ptr() + 4)):
        with pytest.raises(B.KbjError, match="16-byte aligned"):
            ctx.tracking_stats(*args)
    with pytest.raises(B.KbjError, match="settle_steps"):
        ctx.tracking_stats(traj.c, -1, acc, stats)
    names = [k["name"] for k in ctx.profile_end()["kernels"]]
    assert not any("tracking_stats" in n for n in names), names
    assert (stats.cpu().numpy() == -1).all() and not acc.any()
    ctx.profile_begin()
    ctx.tracking_stats(traj.c, 0, acc, stats, err)
    kernels = {k["name"]: k["launches"] for k in ctx.profile_end()["kernels"]}
    assert kernels == {"kbj::tracking_stats_kernel": 1}
    assert stats.cpu().numpy()[L.CMODE["STAND"] * K["MODE_STRIDE"] + K["ROWS"]] == 8       # zero rows: eight standing rows


def test_same_inputs_give_identical_bytes(ctx):
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    T, N = TR.SHAPES[3]
    traj = TrajBuffers(T, N, 64, 2, dev)
    traj.aux.copy_(torch.from_numpy(TR.problems(T, N).calls[1]))
    start = torch.zeros(N, A["SIZE"], device=dev)          # the carry the first call's last row leaves, held for four rows
    start[:, A["CMD"]:A["CMD"] + L.NCMD] = torch.from_numpy(TR.problems(T, N).calls[0][T - 1, :, X["CMD"]:X["CMD"] + L.NCMD].copy()).to(dev)
    start[:, A["SINCE"]], start[:, A["RUNNING"]] = 4.0, 1.0
    outs = []
    for with_err in (True, False, True):
        acc, stats = start.clone(), torch.zeros(K["SIZE"], dtype=torch.float64, device=dev)
        err = torch.zeros(T, N, R["SIZE"], device=dev) if with_err else None
        ctx.tracking_stats(traj.c, 2, acc, stats, err)
        outs.append((acc.cpu().numpy().tobytes(), stats.cpu().numpy().tobytes(), err.cpu().numpy().tobytes() if with_err else None))
    assert outs[0] == outs[2] and outs[0][:2] == outs[1][:2]
