"""CPU tests of the env step's parity by regime (tests/regime_cases.py: quiet stance, every joint limit, the actuator force-range clamp) on the kernel
BODY compiled as a host emulation (tests/emu, the register solver), with the liveness of every case from the oracle alone and the power of the
rule against data mutants. The GPU run of the kernel by the same rule is tests/test_gpu_env_regimes.py.

Figures of a run (`-s`) are tabulated in EXPERIMENTS.md "Env step parity by regime"."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import helpers as H
from tests import regime_cases as R


def _emu(model=None, ep_scale=None):
    """The emulation as a stepper factory; `model`: a mutant that replaces the case's; ep_scale (column, width, factor): the parameter rows the
    emulation (alone) runs on."""
    def factory(m, cfg, seed):
        step = H.emu_stepper(model or m, cfg, seed, lib=H.emu_lib("reg"))
        if ep_scale is None:
            return step
        c0, w, f = ep_scale

        def mutated(ep0, es0, act, aux_in):
            ep = ep0.copy()
            ep[:, c0:c0 + w] *= np.float32(f)
            return step(ep, es0, act, aux_in)
        return mutated
    return factory


@pytest.mark.parametrize("case,robot", R.RUNS)
def test_regime_steps_match_oracle(case, robot):
    """The rule on the emulation; it needs no DONE exemption in any case."""
    res = R.run_case(case, robot, _emu(), label="emu ").check(f"emu {case} {robot}: ")
    assert res.exempted == 0


@pytest.mark.parametrize("case,robot", R.RUNS)
def test_regime_cases_are_live(case, robot):
    """The conditions that make a case a test of its regime, from the oracle alone, and the pinned figures half of which the GPU test asserts."""
    lv = R.check_liveness(case, robot)
    pin = R.MEASURED[(case, robot)]
    print(f"{case} {robot}: ", {k: v for k, v in lv.items() if not isinstance(v, dict)})
    if case != "stance":
        print("  groups below 1.00:", {(g % 20, g // 20): round(v, 3) for g, v in lv["moved"].items() if v < 1})
    for k, v in pin.items():
        assert abs(lv[k] - v) <= 5e-4 * max(1.0, abs(v)), (case, robot, k, lv[k], v)
    assert not R.EXCLUDED.get(case)            # all 40 sides are asserted live


LIMIT_MUTANTS = [(0, 0), (7, 1), (12, 1), (19, 0)]
CLAMP_MUTANTS = [(0, 0), (12, 1)]


def _only_group_fails(res, joint, side, label):
    g = R.group_of(joint, side)
    print(f"{label}: score {res.score[g]:.1f} in its group, at most {max(v for k, v in res.score.items() if k != g):.2f} elsewhere (bound {R.F_GROUP})")
    assert list(res.group) == [g], (label, res.group)
    return res.score[g]


@pytest.mark.parametrize("joint,side", LIMIT_MUTANTS)
def test_limit_mutant_fails_its_group_only(model, joint, side):
    """A model whose limit of one joint on one side is off by 1e-4 rad, given to the emulation: rejected by the per-group rule in that group and
    in no other."""
    res = R.run_case("limits", "kbot-headless", _emu(R.shifted_limit(model, joint, side)), verbose=False)
    _only_group_fails(res, joint, side, f"limit of joint {joint} side {side} + 1e-4 rad")


@pytest.mark.parametrize("joint,side", CLAMP_MUTANTS)
def test_act_range_mutant_fails_its_group_only(model, joint, side):
    """act_range of one joint on one side x 1.001."""
    res = R.run_case("clamp", "kbot-headless", _emu(R.scaled_act_range(model, joint, side, 1.001)), verbose=False)
    _only_group_fails(res, joint, side, f"act_range of joint {joint} side {side} x 1.001")


def test_fricloss_mutant_fails_the_stance():
    """ep[KBJ_EP_FRICLOSS] x 1.01 on the emulation's side only: the pooled rule of the stance case rejects it (its friction-loss rows are inside
    their quadratic zone, where the loss matters)."""
    res = R.run_case("stance", "kbot-headless", _emu(ep_scale=(L.EP["FRICLOSS"], 26, 1.01)), skip_ep=True, verbose=False)
    print("fricloss x 1.01:", res.pooled)
    assert res.pooled and not res.exact


@pytest.mark.parametrize("joint", [7, 12])
def test_older_case_accepts_the_limit_mutants(model, joint):
    """Why these cases exist: the comparison every older parity test of the env step makes (128 envs, 30 steps, "sampler": a reset followed by
    random_actions(scale=0.3), held to helpers.TOL) does not see a model whose upper limit of joint 7 or 12 is off by 1e-4 rad in the physics -
    neither joint ever reaches that limit there: the state errors stay inside helpers.TOL and DONE, ep, counters, ACT_PREV and push wrench are
    the oracle's. The limits case rejects both (test_limit_mutant_fails_its_group_only). Joint 7 (a leg) passes the older case altogether. Joint 12
    is an arm joint, and the command sampler draws the arm targets from dof_range: the command block of the 5 env-steps that resample an arm
    command differs by the 1e-4 rad x u of the draw. That is the sampler's reading of the range, not the limit row ROW_LIM + 12 of the solver,
    which stays unexercised: pinned here as it is, so the record says which part of the older case notices what."""
    assert R.sampler_case_verdict(_emu()) == dict(states=True, exact=True, command=True)
    assert R.sampler_case_verdict(_emu(R.shifted_limit(model, joint, 1))) == dict(states=True, exact=True, command=joint < 10)
