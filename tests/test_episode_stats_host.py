"""Episode statistics, the parts that need no GPU: the host restatement of kbj_episode_stats pinned on a hand-computed case, the layout
mirrors, combining vectors (pure and over gloo), the scalars, the config field and the checkpoint members."""
import dataclasses
import os

import numpy as np
import torch
import torch.multiprocessing as mp

from kbot_joystick_amd.spec import layout as L
from tests import episode_stats_ref as R

E, A, X = L.EPST, L.EACC, L.AUX


def _random_problem(seed, T, N, p_done=0.3):
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-1, 2, (T, N)).astype(np.float32)
    comps = rng.uniform(0, 1, (T, N, L.NREW)).astype(np.float32)
    aux = np.zeros((T, N, X["SIZE"]), np.float32)
    aux[:, :, X["DONE"]] = np.where(rng.random((T, N)) < p_done, rng.choice(np.array([-1, 1, -3.5, 2], np.float32), (T, N)), 0)
    aux[:, :, X["BASEZ"]] = rng.uniform(0.3, 1.0, (T, N))
    aux[:, :, X["LFZ"]] = rng.uniform(0.0, 0.3, (T, N))
    aux[:, :, X["RFZ"]] = rng.uniform(0.0, 0.3, (T, N))
    return reward, aux, comps


def test_layout_mirrors_the_header():
    # (values against the header: tests/test_abi_mirror.py)
    assert E["SIZE"] >= 24 and E["TERM_SUM"] + L.NREW <= E["SIZE"] and A["TERM"] + L.NREW <= A["SIZE"]
    slots = [E[k] for k in E if k not in ("SIZE", "TERM_SUM")] + list(range(E["TERM_SUM"], E["TERM_SUM"] + L.NREW))
    assert len(set(slots)) == len(slots)


def test_hand_computed_case():
    """T = 3, N = 2, unhealthy_z = 0.4. env 0: rewards (1, 2, 4), done (0, +1, 0); env 1: rewards (0.5, 0.25, 8), done (-1, 0, -1) with
    BASEZ - min(LFZ, RFZ) = 0.3 at step 0 (a height failure) and 0.9 at step 2 (another failure)."""
    reward = np.array([[1, 0.5], [2, 0.25], [4, 8]], np.float32)
    aux = np.zeros((3, 2, X["SIZE"]), np.float32)
    aux[:, :, X["DONE"]] = np.array([[0, -1], [1, 0], [0, -1]], np.float32)
    aux[0, 1, X["BASEZ"]], aux[0, 1, X["LFZ"]], aux[0, 1, X["RFZ"]] = 0.8, 0.5, 0.6
    aux[2, 1, X["BASEZ"]], aux[2, 1, X["LFZ"]], aux[2, 1, X["RFZ"]] = 1.0, 0.2, 0.1
    acc = np.zeros((2, A["SIZE"]), np.float32)
    st, _ = R.episode_stats_ref(acc, reward, aux, None, 0.4)
    want = dict(EPISODES=3, FAIL_HEIGHT=1, FAIL_OTHER=1, TRUNCATED=1, RETURN_SUM=11.75, RETURN_SUMSQ=77.3125, RETURN_MIN=0.5, RETURN_MAX=8.25,
                LENGTH_SUM=5, LENGTH_MAX=2, FAIL_LENGTH_SUM=3)
    for k, v in want.items():
        assert st[E[k]] == v, (k, st[E[k]], v)
    assert np.all(st[E["TERM_SUM"]:E["TERM_SUM"] + L.NREW] == 0)
    assert (acc[0, A["RETURN"]], acc[0, A["LENGTH"]]) == (4.0, 1.0) and (acc[1, A["RETURN"]], acc[1, A["LENGTH"]]) == (0.0, 0.0)
    assert np.all(acc[:, A["TERM"]:] == 0)
    # the reward terms ride along: with comps = 1 everywhere an episode's term sums equal its length
    acc = np.zeros((2, A["SIZE"]), np.float32)
    st, _ = R.episode_stats_ref(acc, reward, aux, np.ones((3, 2, L.NREW), np.float32), 0.4)
    assert np.all(st[E["TERM_SUM"]:E["TERM_SUM"] + L.NREW] == 5.0) and np.all(acc[0, A["TERM"]:A["TERM"] + L.NREW] == 1.0)
    # nothing finished: the identities
    st, _ = R.episode_stats_ref(np.zeros((2, A["SIZE"]), np.float32), reward[:1], np.zeros((1, 2, X["SIZE"]), np.float32), None, 0.4)
    assert st[E["EPISODES"]] == 0 and st[E["RETURN_MIN"]] == np.inf and st[E["RETURN_MAX"]] == -np.inf and st[E["LENGTH_MAX"]] == 0


def test_a_height_equal_to_the_threshold_is_not_a_height_failure():
    aux = np.zeros((1, 2, X["SIZE"]), np.float32)
    aux[0, :, X["DONE"]] = -1
    aux[0, :, X["BASEZ"]] = (0.5, np.nextafter(np.float32(0.5), np.float32(0)))
    st, _ = R.episode_stats_ref(np.zeros((2, A["SIZE"]), np.float32), np.ones((1, 2), np.float32), aux, None, 0.5)
    assert (st[E["FAIL_HEIGHT"]], st[E["FAIL_OTHER"]]) == (1, 1)


def test_combine_halves_equals_the_whole():
    from kbot_joystick_amd.host import dist as D
    reward, aux, comps = _random_problem(5, 9, 40)
    whole, mags = R.episode_stats_ref(np.zeros((40, A["SIZE"]), np.float32), reward, aux, comps, 0.4)
    halves = [R.episode_stats_ref(np.zeros((20, A["SIZE"]), np.float32), reward[:, s], aux[:, s], comps[:, s], 0.4)[0] for s in (slice(0, 20), slice(20, 40))]
    assert whole[E["EPISODES"]] > 20 and min(whole[E["FAIL_HEIGHT"]], whole[E["FAIL_OTHER"]], whole[E["TRUNCATED"]]) > 0
    R.assert_stats_match(D.combine_episode_stats(halves), whole, mags)
    assert np.array_equal(D.combine_episode_stats([]), D.empty_episode_stats())
    assert np.array_equal(D.combine_episode_stats([halves[0], D.empty_episode_stats()]), halves[0])


def _reduce_worker(rank, world, port, out):
    import torch.distributed as dist
    from kbot_joystick_amd.host import dist as D
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    reward, aux, comps = _random_problem(5, 9, 40)
    s = slice(20 * rank, 20 * rank + 20)
    mine, _ = R.episode_stats_ref(np.zeros((20, A["SIZE"]), np.float32), reward[:, s], aux[:, s], comps[:, s], 0.4)
    both = np.stack([mine, D.empty_episode_stats() if rank else mine])          # a batch of vectors; rank 1's second one is empty
    out[rank] = dict(mine=mine, reduced=D.reduce_episode_stats(torch.from_numpy(both), world).numpy())
    dist.destroy_process_group()


def test_reduce_episode_stats_two_ranks_gloo():
    from kbot_joystick_amd.host import dist as D
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_reduce_worker, args=(2, 29551, out), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    assert np.array_equal(r0["reduced"], r1["reduced"])
    assert np.array_equal(r0["reduced"][0], D.combine_episode_stats([r0["mine"], r1["mine"]]))     # the same arithmetic, in rank order
    assert np.array_equal(r0["reduced"][1], r0["mine"])
    assert np.array_equal(D.reduce_episode_stats(torch.from_numpy(r0["mine"]), 1).numpy(), r0["mine"])   # one rank: no collective


def test_scalars_of_a_vector():
    from kbot_joystick_amd.host.task import episode_stats_scalars
    from kbot_joystick_amd.host import dist as D
    from kbot_joystick_amd.spec import constants
    assert episode_stats_scalars(D.empty_episode_stats(), 0.02) == {"episode/count": 0.0}
    v = D.empty_episode_stats()
    for k, x in dict(EPISODES=3, FAIL_HEIGHT=1, FAIL_OTHER=1, TRUNCATED=1, RETURN_SUM=11.75, RETURN_SUMSQ=77.3125, RETURN_MIN=0.5, RETURN_MAX=8.25,
                     LENGTH_SUM=5, LENGTH_MAX=2, FAIL_LENGTH_SUM=3).items():
        v[E[k]] = x
    v[E["TERM_SUM"] + 1] = 6.0
    s = episode_stats_scalars(v, 0.02, "x/", terms=True)
    mean = 11.75 / 3
    want = {"x/count": 3.0, "x/return_mean": mean, "x/return_std": (77.3125 / 3 - mean * mean) ** 0.5, "x/return_min": 0.5, "x/return_max": 8.25,
            "x/length_s_mean": 5 / 3 * 0.02, "x/length_s_max": 0.04, "x/time_to_failure_s_mean": 0.03, "x/frac_fail_height": 1 / 3,
            "x/frac_fail_other": 1 / 3, "x/frac_truncated": 1 / 3}
    for k, x in want.items():
        assert abs(s[k] - x) < 1e-12, (k, s[k], x)
    assert s[f"x/reward/{constants.REWARD_NAMES[1]}"] == 2.0 and s[f"x/reward/{constants.REWARD_NAMES[0]}"] == 0.0
    assert set(s) == set(want) | {f"x/reward/{n}" for n in constants.REWARD_NAMES}
    v[E["FAIL_HEIGHT"]] = v[E["FAIL_OTHER"]] = 0
    assert "x/time_to_failure_s_mean" not in episode_stats_scalars(v, 0.02, "x/")


def test_config_field_and_checkpoint_members(tmp_path):
    from kbot_joystick_amd.host import ckpt, dist as D
    from kbot_joystick_amd.host.task import HumanoidWalkingTaskConfig, launch_config
    assert HumanoidWalkingTaskConfig().episode_stats is False and launch_config().episode_stats is False
    cfg = launch_config(episode_stats=True, hidden_size=16, depth=1)
    d = dataclasses.asdict(cfg)
    assert d["episode_stats"] is True
    d["action_latency_range"] = tuple(d["action_latency_range"])
    assert HumanoidWalkingTaskConfig(**d) == cfg
    old = {k: v for k, v in d.items() if k != "episode_stats"}                      # a config member written before the field existed
    assert HumanoidWalkingTaskConfig(**old).episode_stats is False
    P = sum(L.param_count(16, 1))
    p = np.arange(P, dtype=np.float32)
    d["action_latency_range"] = list(d["action_latency_range"])
    acc = np.random.default_rng(0).uniform(0, 9, (4, A["SIZE"])).astype(np.float32)
    total = D.empty_episode_stats()
    total[E["EPISODES"]], total[E["RETURN_SUM"]] = 7, 0.1 + 0.2
    without, with_ = str(tmp_path / "old.bin"), str(tmp_path / "new.bin")
    ckpt.save_ckpt(without, p, p, p, 1, 16, 1, dict(num_steps=1), d, dict(es=np.zeros((4, L.ES["SIZE"]), np.float32)))
    ckpt.save_ckpt(with_, p, p, p, 1, 16, 1, dict(num_steps=1), d, dict(es=np.zeros((4, L.ES["SIZE"]), np.float32), ep_acc=acc, ep_total=total))
    x = ckpt.load_ckpt(without, "all")["extras"]
    assert "ep_acc" not in x and "ep_total" not in x and "es" in x
    z = ckpt.load_ckpt(with_, "all")
    assert z["config"]["episode_stats"] is True
    assert z["extras"]["ep_acc"].dtype == np.float32 and np.array_equal(z["extras"]["ep_acc"], acc)
    assert z["extras"]["ep_total"].dtype == np.float64 and np.array_equal(z["extras"]["ep_total"], total)
