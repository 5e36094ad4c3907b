"""GPU tests of the Polak-Ribiere CG constraint solver (kbj_config.solver_newton = 0; env_step_cg_kernel and the CG forms of the reset-type
kernels) through the C ABI, by the acceptance rule of tests/cg_cases.py; the host emulation of the same source is held to it on the CPU in
tests/test_emu_env_cg.py. Run with `pytest -m gpu` on an MI355X. Figures of a run (`-s`): EXPERIMENTS.md "CG solver against the oracle"."""
import os

import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import cg_cases as CG
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _ctx(model, cfg, lib=None):
    import torch
    from kbot_joystick_amd.host import binding as B
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return B.Context(model, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream, lib=lib), torch


def _obs(torch, N):
    dev = "cuda:0"
    return (torch.zeros(N, L.LD_ACTOR, device=dev), torch.zeros(N, L.LD_CRITIC, device=dev), torch.zeros(N, L.AUX["SIZE"], device=dev))


def _lds_library():
    """The same ABI built with the LDS formulation of the solver, as tests/test_gpu_env.py loads it."""
    import subprocess
    from kbot_joystick_amd.host import binding as B
    csrc = os.path.dirname(B.LIB_PATH)
    subprocess.check_call(["make", "-C", csrc, "-s", "ldssolver"])
    return B.load_library_at(os.path.join(csrc, "libkbj_ldssolver.so"))


def _hip_stepper(lib=None):
    """helpers.emu_stepper's counterpart on the device: env_set_state / env_step as test_teacher_forced_steps_match_oracle drives them."""
    def factory(model, cfg, seed):
        ctx, torch = _ctx(model, cfg, lib)
        N = cfg.num_envs
        a, c, x = _obs(torch, N)
        a2, c2, x2 = _obs(torch, N)
        ctx.env_reset_all(seed, a, c, x)                             # sets the context's seed; the state is overwritten before every step

        def step(ep0, es0, act, aux_in):
            ctx.env_set_state(ep0, es0)
            aux_t = torch.from_numpy(aux_in.copy()).cuda()
            ctx.env_step(torch.from_numpy(np.array(act, np.float32)).cuda(), aux_t, a2, c2, x2)
            ctx.synchronize()
            ep, es = ctx.env_get_state()
            return H.Step(ep, es, aux_t.cpu().numpy(), a2.cpu().numpy(), c2.cpu().numpy(), x2.cpu().numpy())
        step.ctx = ctx
        return step
    return factory


@pytest.mark.parametrize("robot,N,cap,terrain", [("kbot-headless", 256, 2, False), ("kbot-headless", 256, 3, False), ("kbot-headless", 256, 8, False),
                                                 ("kbot-headless", 256, 256, False), ("kbot", 128, 3, True), ("kbot", 128, 8, True)])
def test_cg_steps_match_oracle(robot, N, cap, terrain):
    """env_step_cg_kernel by the rule, at every cap on kbot-headless and at caps 3 and 8 on the full kbot on the sine terrain (BASELINE configs[4])."""
    CG.run_case(robot, N, cap, _hip_stepper(), terrain=terrain, label=f"hip {robot}{' sine' if terrain else ''} ")


def test_cg_steps_match_oracle_lds_build():
    """The LDS formulation of the CG solver on the device (libkbj_ldssolver.so serves both solvers), cap 8."""
    CG.run_case("kbot-headless", 128, 8, _hip_stepper(_lds_library()), label="hip lds build ")


@pytest.mark.parametrize("robot", ["kbot-headless", "kbot"])
def test_cg_reset_matches_oracle(robot):
    def reset(model, cfg, seed):
        ctx, torch = _ctx(model, cfg)
        a, c, x = _obs(torch, cfg.num_envs)
        ctx.env_reset_all(seed, a, c, x)
        ctx.synchronize()
        ep, es = ctx.env_get_state()
        ctx.close()
        return ep, es, a.cpu().numpy(), c.cpu().numpy(), x.cpu().numpy()
    CG.reset_case(robot, 64, reset, label=f"hip {robot} ")


def _free_run(ctx, torch, model, N, steps, seed, record=False):
    """`steps` control steps from a reset with fixed random actions: (state rows, observation / aux rows, state records) after every step."""
    a, c, x = _obs(torch, N)
    a2, c2, x2 = _obs(torch, N)
    ctx.env_reset_all(seed, a, c, x)
    rng = np.random.default_rng(3)
    out = []
    for t in range(steps):
        act = torch.from_numpy(H.random_actions(model, rng, N)).cuda()
        q = torch.zeros(N, L.QSTATE["SIZE"], device="cuda:0") if record else None
        ctx.env_step(act, x, a2, c2, x2, qstate_t=q)
        ctx.synchronize()
        ep, es = ctx.env_get_state()
        out.append((ep, es, x.cpu().numpy(), a2.cpu().numpy(), c2.cpu().numpy(), x2.cpu().numpy(), None if q is None else q.cpu().numpy()))
        x, x2 = x2, x
    return out


def test_cg_recording_twin_is_bit_identical(model):
    """env_step_record_cg_kernel leaves the states env_step_cg_kernel leaves, bit for bit, and its record is the state after the step."""
    N = 64
    cfg = CG.cg_config(N, 8)
    runs = []
    for record in (False, True):
        ctx, torch = _ctx(model, cfg)
        runs.append(_free_run(ctx, torch, model, N, 4, 7, record))
        ctx.close()
    for plain, rec in zip(*runs):
        for p, r in zip(plain[:6], rec[:6]):
            assert np.array_equal(p.view(np.uint32), r.view(np.uint32))
        done = plain[2][:, L.AUX["DONE"]] != 0
        assert np.array_equal(rec[6][~done, L.QSTATE["QPOS"]:L.QSTATE["QPOS"] + 27], rec[1][~done, 0:27])
        assert np.array_equal(rec[6][~done, L.QSTATE["QVEL"]:L.QSTATE["QVEL"] + 26], rec[1][~done, 28:54])


@pytest.mark.parametrize("T", [5, 6])
def test_cg_fused_rollout_equals_stepwise_calls(model, T):
    """Invariant 5 under CG: kbj_rollout equals kbj_policy_step / kbj_env_step / kbj_carry_reset one call at a time, bit for bit; T = 5 and 6 are
    the two parities of the rollout's h-plane alternation."""
    import torch
    from kbot_joystick_amd.host import buffers
    N, Hh = 64, 64
    cfg = CG.cg_config(N, 8, rollout_len=T, hidden_size=Hh)
    out = []
    for mode in ("fused", "stepwise"):
        ctx, _ = _ctx(model, cfg)
        params = torch.zeros(ctx.param_count(), device="cuda:0")
        ctx.init_params(9, params)
        carry = buffers.CarryBuffers(N, Hh, 2, "cuda:0")
        tr = buffers.TrajBuffers(T, N, Hh, 2, "cuda:0")
        ctx.env_reset_all(3, tr.actor_obs[T], tr.critic_obs[T], tr.aux[T])
        for it in range(2):
            if mode == "fused":
                ctx.rollout(params, carry.c, 3, it * T, tr.c)
            else:
                tr.actor_obs[0].copy_(tr.actor_obs[T]); tr.critic_obs[0].copy_(tr.critic_obs[T]); tr.aux[0].copy_(tr.aux[T])
                for t in range(T):
                    ctx.policy_step(params, tr.actor_obs[t], tr.critic_obs[t], carry.c, 3, it * T + t, False, tr.action[t], tr.logp[t], tr.value[t])
                    ctx.env_step(tr.action[t], tr.aux[t], tr.actor_obs[t + 1], tr.critic_obs[t + 1], tr.aux[t + 1])
                    ctx.carry_reset(carry.c, tr.aux[t].data_ptr() + 4 * L.AUX["DONE"], L.AUX["SIZE"])
                ctx.rewards(tr.aux, T, tr.reward)
        ctx.synchronize()
        ep, es = ctx.env_get_state()
        out.append([tr.actor_obs.clone(), tr.critic_obs.clone(), tr.aux.clone(), tr.action.clone(), tr.logp.clone(), tr.value.clone(), tr.reward.clone(),
                    carry.actor_hc.clone(), carry.critic_hc.clone(), carry.lpf.clone(), torch.from_numpy(es.view(np.int32))])
        ctx.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert torch.isfinite(out[0][6]).all()


def test_cg_task_trains_and_validates():
    """solver="cg" through the task: two training iterations to finite losses, and the validation context inherits the solver."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
    cfg = launch_config(num_envs=64, batch_size=32, hidden_size=64, rollout_length_seconds=8 * 0.02, robot="kbot-headless", seed=2, num_passes=1, solver="cg")
    task = HumanoidWalkingTask(cfg)
    assert task.kcfg.solver_newton == 0 and task.T == 8
    for _ in range(2):
        task.train_iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(task.metrics).all() and torch.isfinite(task.params).all() and torch.isfinite(task.traj.reward).all()
    stats = task.validate(num_envs=64, seconds=0.1)
    assert task._valid[1].config.solver_newton == 0
    assert all(np.isfinite(v) for v in stats.values() if isinstance(v, float))
    task._valid[1].close()
    task.ctx.close()


def test_solver_is_selected_per_context(model):
    """A Newton context created after a CG context in the same process gives the rows of one created alone: the solver is the context's."""
    N = 64
    newton = L.default_config(num_envs=N, batch_size=N)
    ctx, torch = _ctx(model, newton)
    alone = _free_run(ctx, torch, model, N, 3, 5)
    ctx.close()
    cg_ctx, _ = _ctx(model, CG.cg_config(N, 8))
    cg = _free_run(cg_ctx, torch, model, N, 3, 5)
    ctx, _ = _ctx(model, newton)                                      # while the CG context is alive
    after = _free_run(ctx, torch, model, N, 3, 5)
    ctx.close(); cg_ctx.close()
    for x, y in zip(alone, after):
        for p, r in zip(x[:6], y[:6]):
            assert np.array_equal(p.view(np.uint32), r.view(np.uint32))
    assert not np.array_equal(alone[-1][1][:, 28:54], cg[-1][1][:, 28:54])      # and CG is another dynamics: the two runs differ
