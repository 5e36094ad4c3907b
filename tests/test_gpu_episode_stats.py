"""kbj_episode_stats on the GPU: synthetic trajectories through the C ABI against the host restatement (tests/episode_stats_ref.py),
bit-reproducibility, and the feature end to end through HumanoidWalkingTask (rollouts, scalars, validation, checkpoint, off = off).

Bounds. Accumulators: bit-equal (the ABI fixes the order of the fp32 adds). Counts, minimum, maximum, longest episode: exact. Every double
sum: within 1e-9 * sum |x_i| of math.fsum - double accumulation of at most ~2,000 fp32 values errs by at most count * 2^-53 * sum |x| ~
2e-13 * sum |x| whatever the reduction tree; the margin is not a measured tolerance. Conservation: the returns of the finished episodes
plus the running ones equal the float64 sum of all rewards within 1e-5 * sum |r| (fp32 accumulation over <= 24 adds per env)."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import episode_stats_ref as R

pytestmark = pytest.mark.gpu
E, A, X = L.EPST, L.EACC, L.AUX
UZ = 0.4
SHAPES = [(1, 1), (7, 65), (8, 96), (5, 130)]      # a lone env; ragged last blocks of 1 and of 32 envs; more than two blocks


@pytest.fixture(scope="module")
def ctx():
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.spec import compiler
    c = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=64, batch_size=64, hidden_size=64, rollout_len=8, unhealthy_z=UZ))
    yield c
    c.close()


def _problem(rng, T, N):
    """Random rewards / terms / DONE / heights in the normal range, with the corner cases planted: DONE at t = 0 for env 0 (a failure whose
    height EQUALS the threshold: not a height failure under <), DONE at t = T - 1 for the last env, two consecutive DONE steps for env 1 and
    no DONE at all for env 2 (when there are that many envs and steps)."""
    reward = rng.uniform(-1, 2, (T, N)).astype(np.float32)
    comps = rng.uniform(0.01, 1, (T, N, L.NREW)).astype(np.float32)
    aux = np.zeros((T + 1, N, X["SIZE"]), np.float32)
    done = np.where(rng.random((T, N)) < 0.3, rng.choice(np.array([-1, 1, -3.5, 2], np.float32), (T, N)), 0).astype(np.float32)
    bz, lf, rf = rng.uniform(0.2, 0.9, (T, N)), rng.uniform(0.0, 0.3, (T, N)), rng.uniform(0.0, 0.3, (T, N))
    done[T - 1, N - 1] = -1
    if N >= 4:
        if T >= 3:
            done[1, 1], done[2, 1] = -3.5, 2
        done[:, 2] = 0
    done[0, 0] = -1
    bz[0, 0], lf[0, 0], rf[0, 0] = np.float32(UZ), 0.0, 0.1
    aux[:T, :, X["DONE"]], aux[:T, :, X["BASEZ"]], aux[:T, :, X["LFZ"]], aux[:T, :, X["RFZ"]] = done, bz, lf, rf
    return reward, aux, comps


def _upload(traj, reward, aux, comps):
    import torch
    traj.reward.copy_(torch.from_numpy(reward)); traj.aux.copy_(torch.from_numpy(aux))
    if traj.comps is not None:
        traj.comps.copy_(torch.from_numpy(comps))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("T,N", SHAPES)
def test_synthetic_trajectories_match_the_restatement(ctx, T, N):
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    for with_comps in (False, True):
        rng = np.random.default_rng(1000 * T + N)
        traj = TrajBuffers(T, N, 64, 2, dev, reward_comps=with_comps)
        acc_ref = np.zeros((N, A["SIZE"]), np.float32)
        acc_ref[:, A["TERM"] + L.NREW:] = 7.0                     # the spare floats of a row are left alone
        acc = torch.from_numpy(acc_ref.copy()).to(dev)
        stats = torch.full((E["SIZE"],), -1.0, dtype=torch.float64, device=dev)       # overwritten, spare slots included
        ret_total, all_r, all_abs, seen = 0.0, 0.0, 0.0, np.zeros(E["SIZE"])
        for call in range(3):
            reward, aux, comps = _problem(rng, T, N)
            _upload(traj, reward, aux, comps)
            ctx.episode_stats(traj.c, acc, stats)
            want, mags = R.episode_stats_ref(acc_ref, reward, aux, comps if with_comps else None, UZ)
            got = stats.cpu().numpy()
            print(f"T={T} N={N} comps={with_comps} call={call}: episodes {got[E['EPISODES']]:.0f} (height {got[E['FAIL_HEIGHT']]:.0f}, other {got[E['FAIL_OTHER']]:.0f}, "
                  f"truncated {got[E['TRUNCATED']]:.0f}) return_sum err {abs(got[E['RETURN_SUM']] - want[E['RETURN_SUM']]):.2e} (bound {1e-9 * mags['RETURN_SUM']:.2e})")
            assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc_ref)), "accumulators differ from the float32 loop"
            R.assert_stats_match(got, want, mags)
            if not with_comps:
                assert np.all(got[E["TERM_SUM"]:E["TERM_SUM"] + L.NREW] == 0) and np.all(acc_ref[:, A["TERM"]:A["TERM"] + L.NREW] == 0)
            ret_total += got[E["RETURN_SUM"]]
            all_r += float(reward.astype(np.float64).sum()); all_abs += float(np.abs(reward.astype(np.float64)).sum())
            seen += got
        live = float(acc.cpu().numpy()[:, A["RETURN"]].astype(np.float64).sum())
        assert abs(ret_total + live - all_r) <= 1e-5 * all_abs, (ret_total, live, all_r)
        assert seen[E["FAIL_OTHER"]] >= 3                       # the planted height == threshold failure, once per call
        if N > 1:
            assert seen[E["FAIL_HEIGHT"]] > 0 and seen[E["TRUNCATED"]] > 0, seen[:4]


def test_null_arguments_fail_with_a_message(ctx):
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    traj = TrajBuffers(2, 4, 64, 2, dev)
    acc, stats = torch.zeros(4, A["SIZE"], device=dev), torch.zeros(E["SIZE"], dtype=torch.float64, device=dev)
    for args in ((traj.c, None, stats), (traj.c, acc, None)):
        with pytest.raises(B.KbjError, match="null argument"):
            ctx.episode_stats(*args)
    with pytest.raises(B.KbjError, match="16-byte aligned"):
        ctx.episode_stats(traj.c, acc.data_ptr() + 4, stats)


def test_same_inputs_give_identical_bytes(ctx):
    import torch
    from kbot_joystick_amd.host.buffers import TrajBuffers
    dev = torch.device("cuda", 0)
    T, N = 8, 96
    rng = np.random.default_rng(9)
    traj = TrajBuffers(T, N, 64, 2, dev, reward_comps=True)
    _upload(traj, *_problem(rng, T, N))
    start = torch.from_numpy(rng.uniform(0, 3, (N, A["SIZE"])).astype(np.float32)).to(dev)
    outs = []
    for _ in range(2):
        acc, stats = start.clone(), torch.zeros(E["SIZE"], dtype=torch.float64, device=dev)
        ctx.episode_stats(traj.c, acc, stats)
        outs.append((acc.cpu().numpy().tobytes(), stats.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def _cfg(**kw):
    from kbot_joystick_amd.host.task import launch_config
    base = dict(num_envs=64, batch_size=64, hidden_size=64, num_passes=1, rollout_length_seconds=8 * 0.02, robot="kbot-headless", seed=5)
    base.update(kw)
    return launch_config(**base)


def test_end_to_end_through_the_task():
    """Every env is truncated after exactly 5 steps whatever the physics does, so with T = 8 every rollout finishes episodes and episodes
    straddle the rollout boundaries."""
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    from kbot_joystick_amd.host import dist as D
    from kbot_joystick_amd.spec import constants
    cfg = _cfg(episode_stats=True, log_reward_components=True, termination_params={"episode_length": {"max_length_sec": 5 * 0.02}})
    task = HumanoidWalkingTask(cfg)
    assert (task.T, task.N, int(task.kcfg.max_episode_steps)) == (8, 64, 5)
    acc_ref = np.zeros((64, A["SIZE"]), np.float32)
    totals = []
    for it in range(3):
        task.train_iteration()
        reward, comps, aux = task.traj.reward.cpu().numpy(), task.traj.comps.cpu().numpy(), task.traj.aux.cpu().numpy()
        want, mags = R.episode_stats_ref(acc_ref, reward, aux, comps, task.kcfg.unhealthy_z)
        last, total = task.episode_stats_vectors()
        assert want[E["EPISODES"]] >= 64 and want[E["TRUNCATED"]] > 0
        R.assert_stats_match(last, want, mags)
        totals.append(want)
        assert np.array_equal(_bits(task.episodes.acc.cpu().numpy()), _bits(acc_ref))
        _, es = task.ctx.env_get_state()
        assert np.array_equal(task.episodes.acc[:, A["LENGTH"]].cpu().numpy(), es[:, L.ES["TIME"]])     # kernel and env agree on where episodes start
        sc = task.scalars()
        assert sc["episode/count"] == want[E["EPISODES"]] and sc["episode_total/count"] == sum(w[E["EPISODES"]] for w in totals)
        assert abs(sc["episode/frac_truncated"] + sc["episode/frac_fail_height"] + sc["episode/frac_fail_other"] - 1.0) < 1e-12
        assert abs(sc["episode/return_mean"] - want[E["RETURN_SUM"]] / want[E["EPISODES"]]) <= 1e-9 * mags["RETURN_SUM"]
        assert sc["episode/length_s_max"] == 5 * cfg.ctrl_dt
        assert all(f"episode/reward/{n}" in sc for n in constants.REWARD_NAMES) and "train/loss" in sc
        assert np.allclose(total, D.combine_episode_stats(totals), rtol=1e-12, atol=0)
    v = task.validate(num_envs=64, seconds=8 * 0.02)
    assert v["valid/episode/count"] >= 64 and v["valid/episode/length_s_max"] == 5 * cfg.ctrl_dt      # fresh accumulators: every env is cut at step 5 of its 8
    assert abs(v["valid/episode/frac_truncated"] + v["valid/episode/frac_fail_height"] + v["valid/episode/frac_fail_other"] - 1.0) < 1e-12
    assert "valid/reward_per_step" in v
    task.close()


def test_every_step_a_height_failure():
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    task = HumanoidWalkingTask(_cfg(episode_stats=True, termination_params={"bad_z": {"unhealthy_z": 10.0}}))
    task.train_iteration()
    sc = task.episode_stats()
    reward = task.traj.reward.cpu().numpy().astype(np.float64)
    assert sc["episode/count"] == 8 * 64 and sc["episode/frac_fail_height"] == 1.0
    assert sc["episode/length_s_max"] == task.config.ctrl_dt and abs(sc["episode/length_s_mean"] - task.config.ctrl_dt) < 1e-15
    assert abs(sc["episode/time_to_failure_s_mean"] - task.config.ctrl_dt) < 1e-15
    assert abs(sc["episode/return_mean"] - reward.mean()) <= 1e-6 * abs(reward.mean())
    assert not any(k.startswith("episode/reward/") for k in sc)           # no log_reward_components: no per-term keys
    assert not task.episodes.acc.any()
    task.close()


def test_checkpoint_carries_the_accounting(tmp_path):
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    cfg = _cfg(episode_stats=True, log_reward_components=True, termination_params={"episode_length": {"max_length_sec": 5 * 0.02}})
    a = HumanoidWalkingTask(cfg)
    for _ in range(2):
        a.train_iteration()
    path = str(tmp_path / "ckpt.bin")
    a.save_checkpoint(path)
    a.train_iteration()
    b = HumanoidWalkingTask(cfg)
    b.load_checkpoint(path)
    b.train_iteration()
    assert a.episodes.acc.any() and torch.equal(a.episodes.acc, b.episodes.acc)
    da, db = a.episode_stats(), b.episode_stats()
    assert da == db and da["episode_total/count"] > da["episode/count"] > 0
    # a checkpoint of a run that did not keep the accounting loads into one that does: it starts from zero
    off = HumanoidWalkingTask(_cfg())
    off.train_iteration()
    path_off = str(tmp_path / "off.bin")
    off.save_checkpoint(path_off)
    b.load_checkpoint(path_off)
    assert not b.episodes.acc.any() and b.episode_stats() == {"episode/count": 0.0, "episode_total/count": 0.0}
    b.train_iteration()
    assert b.episode_stats()["episode_total/count"] == b.episode_stats()["episode/count"]
    for t in (a, b, off):
        t.close()


def test_off_means_off():
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    off, on = HumanoidWalkingTask(_cfg(deterministic=True)), HumanoidWalkingTask(_cfg(deterministic=True, episode_stats=True))
    assert off.episodes is None
    with pytest.raises(B.KbjError, match="episode_stats=True"):
        off.episode_stats()
    off.train_iteration(); on.train_iteration()
    names = ("loss", "policy_loss", "value_loss", "entropy", "clip_fraction", "approx_kl", "adv_mean", "adv_std", "action_mirror_loss", "value_mirror_loss",
             "reward_per_step", "failures_per_step", "truncations_per_step", "value_mean", "action_std_logp")
    assert set(off.scalars()) == {f"train/{n}" for n in names}
    assert set(on.scalars()) - set(off.scalars()) and all(k.startswith(("episode/", "episode_total/")) for k in set(on.scalars()) - set(off.scalars()))
    assert not any(k.startswith("valid/episode/") for k in off.validate(num_envs=64, seconds=0.1))
    for name in ("actor_obs", "critic_obs", "aux", "action", "logp", "value", "reward", "adv", "target"):      # the feature only observes
        assert torch.equal(getattr(off.traj, name), getattr(on.traj, name)), name
    assert torch.equal(off.params, on.params) and torch.equal(off.opt_m, on.opt_m)
    off.close(); on.close()
