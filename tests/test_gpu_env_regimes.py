"""GPU tests of the env step's parity by regime (tests/regime_cases.py: quiet stance, every joint limit, the actuator force-range clamp): env_step_kernel
through the C ABI, teacher-forced against the oracle halves and by the rule the host emulation of the same source is held to on the CPU
(tests/test_emu_env_regimes.py). Run with `pytest -m gpu` on an MI355X. Figures of a run (`-s`): EXPERIMENTS.md "Env step parity by regime"."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import helpers as H
from tests import regime_cases as R

pytestmark = pytest.mark.gpu


def _hip_stepper(model=None):
    """helpers.emu_stepper's counterpart on the device: env_set_state / env_step / env_get_state on a context of its own, which step.close()
    (regime_cases.run_case calls it after the last step) closes. `model`: a mutant the context is created from in place of the case's."""
    def factory(m, cfg, seed):
        import torch
        from kbot_joystick_amd.host import binding as B
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        ctx = B.Context(model or m, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)
        N, dev = cfg.num_envs, "cuda:0"
        a, c, x = (torch.zeros(N, w, device=dev) for w in (L.LD_ACTOR, L.LD_CRITIC, L.AUX["SIZE"]))
        a2, c2, x2 = (torch.zeros(N, w, device=dev) for w in (L.LD_ACTOR, L.LD_CRITIC, L.AUX["SIZE"]))
        ctx.env_reset_all(seed, a, c, x)                             # sets the context's seed; the state is overwritten before every step

        def step(ep0, es0, act, aux_in):
            ctx.env_set_state(ep0, es0)
            aux_t = torch.from_numpy(aux_in.copy()).cuda()
            ctx.env_step(torch.from_numpy(np.array(act, np.float32)).cuda(), aux_t, a2, c2, x2)
            ctx.synchronize()
            ep, es = ctx.env_get_state()
            return H.Step(ep, es, aux_t.cpu().numpy(), a2.cpu().numpy(), c2.cpu().numpy(), x2.cpu().numpy())
        step.close = ctx.close
        return step
    return factory


@pytest.mark.parametrize("case,robot", R.RUNS)
def test_regime_steps_match_oracle(case, robot):
    """The six runs by the rule, each live by half of the figures the CPU test pins."""
    R.check_liveness(case, robot, half=True)
    R.run_case(case, robot, _hip_stepper(), label="hip ").check(f"hip {case} {robot}: ")


def test_limit_mutant_on_the_device_fails_its_group_only(model):
    """A context created from a model whose upper limit of joint 12 is off by 1e-4 rad fails the rule in group (12, upper) and in no other: the
    device path reads the limit it is given, and the rule sees it there."""
    res = R.run_case("limits", "kbot-headless", _hip_stepper(R.shifted_limit(model, 12, 1)), verbose=False)
    g = R.group_of(12, 1)
    print(f"hip, upper limit of joint 12 + 1e-4 rad: score {res.score[g]:.1f} in its group, at most {max(v for k, v in res.score.items() if k != g):.2f} elsewhere")
    assert list(res.group) == [g], res.group
