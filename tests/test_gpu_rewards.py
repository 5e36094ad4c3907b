"""rewards_kernel through kbj_rewards against the float64 restatement (tests/rewards_ref.py) on the planted cases of tests/rewards_cases.py,
whose census, margins and bounds tests/test_rewards_ref.py proves on the CPU.

What is exact: single_contact, no_contact, the zero / non-zero pattern of feet_airtime, com_distance and torque, on EVERY row (every
threshold of every row has a proven margin); the five carry words after every call, bit for bit the fp32 oracle's; the three spare words of
a carry row, the guard bands around reward and comps, the aux rows: untouched; a call without components, a second context, a trajectory
cut into two calls: the same bits (base_accel at the first row of the second call is exactly 1.0f: the scan edge-pads the velocity).

What is toleranced: every other element, within F[term] x the restatement's condition bound of THAT element. F is not fitted to the kernel:
it is 4 x the largest multiple of the bound the fp32 oracle reaches on these cases on the CPU (EXPERIMENTS.md "Reward stack against the
float64 reference"; tests/test_rewards_ref.py::test_measured_ratio_of_the_fp32_oracle holds the figures to the measurement), the 4 for the
device's 1 to 2 ulp expf / atan2f / asinf / sinf / cosf. The total: the fp32 sum of scale[k] * r[k] over the kernel's OWN components in the
kernel's order, within 12 roundings. Run with -s for the kernel's own largest multiple of the bound per term."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import rewards_cases as CS, rewards_ref as RR

pytestmark = pytest.mark.gpu
X, RC = L.AUX, L.RC

# EXPERIMENTS.md "Reward stack against the float64 reference": 4 x the fp32 oracle's measured ratio (rounded up to a tenth), per term
F_KERNEL = dict(linvel=2.8, angvel=3.2, roll_pitch=3.2, base_height=3.6, arm_pos=2.4, feet_airtime=1.6, feet_orient=2.4, com_distance=2.8,
                base_accel=3.6, torque=4.0)
GUARD, PATTERN = 96, -7.25          # floats before, between and behind reward and comps in their one allocation


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Run:
    """One context of N envs under a case's config, reset (which initialises the reward carry), and kbj_rewards calls with guarded outputs."""

    def __init__(self, case, n):
        import torch
        from kbot_joystick_amd.host import binding as B
        from kbot_joystick_amd.spec import compiler
        self.torch, self.dev, self.n = torch, torch.device("cuda", 0), n
        self.ctx = B.Context(compiler.load_model("kbot-headless"), CS.config(case, n))
        obs = [torch.zeros(n, d, device=self.dev) for d in (L.LD_ACTOR, L.LD_CRITIC, X["SIZE"])]
        self.ctx.env_reset_all(0, *obs)

    def close(self):
        self.ctx.close()

    def call(self, aux, carry=None, comps=True):
        """(comps [T, N, 12] or None, reward [T, N], carry [N, 8]) of one call on rows `aux` (numpy); asserts the guards and aux unchanged."""
        torch, n, T = self.torch, self.n, aux.shape[0]
        if carry is not None:
            self.ctx.env_set_reward_carry(carry)
        aux_d = torch.from_numpy(np.array(aux, np.float32)).to(self.dev)
        nr, nc = T * n, T * n * L.NREW
        flat = torch.full((3 * GUARD + nr + nc,), PATTERN, device=self.dev)
        reward, comps_d = flat[GUARD:GUARD + nr].view(T, n), flat[2 * GUARD + nr:2 * GUARD + nr + nc].view(T, n, L.NREW)
        self.ctx.rewards(aux_d, T, reward, comps_d if comps else None)
        self.ctx.synchronize()
        host = flat.cpu().numpy()
        guards = np.concatenate([host[:GUARD], host[GUARD + nr:2 * GUARD + nr], host[2 * GUARD + nr + nc:]] + ([] if comps else [host[2 * GUARD + nr:]]))
        assert (guards == np.float32(PATTERN)).all(), "kbj_rewards wrote outside reward / comps"
        assert aux_d.cpu().numpy().tobytes() == np.ascontiguousarray(aux).tobytes(), "kbj_rewards changed the aux rows"
        r = host[GUARD:GUARD + nr].reshape(T, n).copy()
        c = host[2 * GUARD + nr:2 * GUARD + nr + nc].reshape(T, n, L.NREW).copy() if comps else None
        return c, r, self.ctx.env_get_reward_carry()


def test_the_factors_are_the_measured_ones():
    assert {RR.NAMES[k]: v for k, v in RR.F.items()} == F_KERNEL


@pytest.mark.parametrize("n", CS.SIZES)
@pytest.mark.parametrize("name", [c.name for c in CS.CASES])
def test_planted_rows_match_the_restatement(model, name, n):
    from oracle import oracle as O
    case = CS.BY_NAME[name]
    aux, rc = case.problem(n)
    ref, P = case.reference(n), RR.Params(CS.config(case, n))
    o = O.Oracle(model, CS.config(case, n), precision="f32")
    o.rc[:] = rc
    o.rewards(aux)
    run = Run(case, n)
    try:
        assert np.array_equal(_bits(run.ctx.env_get_reward_carry()), _bits(RR.initial_carry(n))), "init_reward_carry_kernel"
        got = run.call(aux, rc)
        fails = RR.compare(got, ref, P, carry_want=o.rc)
        assert fails == [], fails
        assert np.array_equal(_bits(got[2][:, 5:]), _bits(rc[:, 5:])), "the spare carry words changed"
        assert np.array_equal(_bits(got[2]), _bits(ref.carry))
        for k, v in RR.ratios(got[0], ref).items():
            print(f"{name} N={n} {RR.NAMES[k]}: kernel reaches {v:.3f} x bound (allowed {RR.F[k]})")
        # without components: the same reward and carry bits
        _, r2, rc2 = run.call(aux, rc, comps=False)
        assert r2.tobytes() == got[1].tobytes() and rc2.tobytes() == got[2].tobytes()
        # a fresh context from the same carry: the same bytes
        other = Run(case, n)
        try:
            again = other.call(aux, rc)
        finally:
            other.close()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got))
    finally:
        run.close()


@pytest.mark.parametrize("n", (65, 130))
def test_a_trajectory_cut_in_two_gives_the_same_bits(n):
    """Rows [0, T) in one call against [0, k) then [k, T) in two, from the same carry (N = 65: a carry no reset leaves), for every k of
    rewards_cases.SPLITS - tests/test_rewards_ref.py::test_carried_words_at_the_split_rows shows what crosses each cut. Everything equal bit
    for bit, but base_accel and the total on row k: there base_accel is exactly 1.0f and the total is the sum of that row's own components."""
    case = CS.BY_NAME["every_branch"]
    aux, rc = case.problem(n)
    P, T = RR.Params(CS.config(case, n)), case.T
    assert CS.SPLITS == (1, 3, 7, T // 2, T - 1)
    whole_run, split_run = Run(case, n), Run(case, n)
    try:
        whole = whole_run.call(aux, rc)
        assert RR.compare(whole, case.reference(n), P) == []
        for k in CS.SPLITS:
            c1, r1, mid = split_run.call(aux[:k], rc)
            c2, r2, end = split_run.call(aux[k:])
            comps, reward = np.concatenate([c1, c2]), np.concatenate([r1, r2])
            assert not np.array_equal(_bits(mid[:, :5]), _bits(end[:, :5]))
            assert np.array_equal(_bits(end), _bits(whole[2])), k
            same = np.ones(comps.shape, bool)
            same[k, :, RR.BASE_ACCEL] = False
            assert np.array_equal(_bits(comps)[same], _bits(whole[0])[same]), k
            assert (comps[k, :, RR.BASE_ACCEL] == np.float32(1.0)).all() and (whole[0][k, :, RR.BASE_ACCEL] < 1).all()
            rows = np.arange(T) != k
            assert np.array_equal(_bits(reward)[rows], _bits(whole[1])[rows]), k
            tot, tb = RR.own_total(comps[k], P)
            assert (np.abs(reward[k].astype(np.float64) - tot) <= tb).all()
    finally:
        whole_run.close(); split_run.close()


def test_bad_arguments_are_refused_and_write_nothing():
    import torch
    from kbot_joystick_amd.host import binding as B
    case, n = CS.BY_NAME["edited_table"], 65
    aux, rc = case.problem(n)
    run = Run(case, n)
    try:
        run.ctx.env_set_reward_carry(rc)
        aux_d = torch.from_numpy(np.array(aux, np.float32)).to(run.dev)
        reward, comps = torch.full((case.T, n), PATTERN, device=run.dev), torch.full((case.T, n, L.NREW), PATTERN, device=run.dev)
        for args in ((aux_d, 0, reward, comps), (aux_d, -3, reward, comps), (None, case.T, reward, comps), (aux_d, case.T, None, comps)):
            with pytest.raises(B.KbjError, match="kbj_rewards: bad arguments"):
                run.ctx.rewards(*args)
        run.ctx.synchronize()
        assert (reward == PATTERN).all() and (comps == PATTERN).all()
        assert np.array_equal(_bits(run.ctx.env_get_reward_carry()), _bits(rc))
    finally:
        run.close()
