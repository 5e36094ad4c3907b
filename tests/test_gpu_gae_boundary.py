"""The selectable GAE boundary conventions on the GPU (kbj_config.gae_bootstrap_truncation / gae_tail_value, include/kbj.h kbj_gae):
kbj_gae against the float64 restatement (tests/gae_ref.py; its liveness on these problems is asserted in tests/test_gae_boundary_host.py),
kbj_critic_value against kbj_policy_step bit for bit and against the oracle, and a whole task with truncations inside every rollout."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import gae_ref as G

pytestmark = pytest.mark.gpu

SWITCHES = [(1, 0), (0, 1), (1, 1)]
DISCOUNTS = [(0.94, 0.94), (1.0, 1.0), (0.9, 0.0)]


def _ctx(N, B, T, H, **kw):
    import torch
    from kbot_joystick_amd.host import binding as Bd
    m = compiler.load_model("kbot-headless")
    cfg = L.default_config(num_envs=N, batch_size=B, rollout_len=T, hidden_size=H, **kw)
    return m, cfg, Bd.Context(m, cfg, 0, torch.cuda.current_stream().cuda_stream)


def _check(label, got_adv, got_tgt, value, reward, done, tail, gamma, lam, bt):
    adv, tgt = G.gae_ref(value, reward, done, gamma, lam, bt, tail)
    bound = G.gae_bound(value, reward, tail, adv, gamma, lam)
    ea, et = np.abs(got_adv.astype(np.float64) - adv).max(), np.abs(got_tgt.astype(np.float64) - tgt).max()
    print(f"{label}: adv err {ea:.3g}, target err {et:.3g}, bound {bound:.3g}")
    assert ea <= bound and et <= bound, (label, ea, et, bound)


@pytest.mark.parametrize("N,T", [(40, 9), (130, 100), (70, 1)])   # a ragged last wavefront; three blocks at the workload's rollout length; the tail-only edge
def test_gae_matches_the_reference(N, T):
    import torch
    from kbot_joystick_amd.host import buffers
    p = G.boundary_problem(N, T)
    tr = buffers.TrajBuffers(T, N, 64, 1, "cuda:0")
    tr.aux[:T, :, L.AUX["DONE"]] = torch.from_numpy(p["done"]).cuda()
    tr.reward.copy_(torch.from_numpy(p["reward"])); tr.value.copy_(torch.from_numpy(p["value"])); tr.value_tail.copy_(torch.from_numpy(p["tail"]))
    for gamma, lam in DISCOUNTS:
        for bt, tv in SWITCHES:
            m, cfg, ctx = _ctx(N, N, T, 64, depth=1, gamma=gamma, lam=lam, gae_bootstrap_truncation=bt, gae_tail_value=tv)
            tr.adv.fill_(float("nan")); tr.target.fill_(float("nan"))
            ctx.gae(tr.c, tr.adv, tr.target)
            ctx.synchronize()
            _check(f"(N, T) = ({N}, {T}) switches ({bt}, {tv}) gamma {gamma} lam {lam}", tr.adv.cpu().numpy(), tr.target.cpu().numpy(), p["value"], p["reward"], p["done"],
                   p["tail"] if tv else None, cfg.gamma, cfg.lam, bt)
            ctx.close()
    # both switches off: the kernel of the default path, reproducible bit for bit, and it never reads the tail
    m, cfg, ctx = _ctx(N, N, T, 64, depth=1)
    tr.value_tail.fill_(float("nan"))
    ctx.gae(tr.c, tr.adv, tr.target)
    a2, t2 = torch.empty_like(tr.adv), torch.empty_like(tr.target)
    ctx.gae(tr.c, a2, t2)
    ctx.synchronize()
    assert torch.equal(tr.adv, a2) and torch.equal(tr.target, t2) and torch.isfinite(a2).all()
    _check(f"(N, T) = ({N}, {T}) default", a2.cpu().numpy(), t2.cpu().numpy(), p["value"], p["reward"], p["done"], None, cfg.gamma, cfg.lam, 0)
    ctx.close()


def test_gae_tail_without_the_array_is_an_error():
    import torch
    from kbot_joystick_amd.host import binding as Bd, buffers
    N, T = 40, 9
    p = G.boundary_problem(N, T)
    m, cfg, ctx = _ctx(N, N, T, 64, depth=1, gae_tail_value=1)
    tr = buffers.TrajBuffers(T, N, 64, 1, "cuda:0")
    tr.aux[:T, :, L.AUX["DONE"]] = torch.from_numpy(p["done"]).cuda()
    tr.reward.copy_(torch.from_numpy(p["reward"])); tr.value.copy_(torch.from_numpy(p["value"])); tr.value_tail.copy_(torch.from_numpy(p["tail"]))
    no_tail = Bd.Traj.from_buffer_copy(tr.c)      # the same pointers, one of them cleared
    no_tail.value_tail_d = None
    tr.adv.fill_(7.0)
    with pytest.raises(Bd.KbjError, match="value_tail_d"):
        ctx.gae(no_tail, tr.adv, tr.target)
    ctx.synchronize()
    assert bool((tr.adv == 7.0).all())            # nothing was launched
    ctx.gae(tr.c, tr.adv, tr.target)              # the context stays usable
    ctx.synchronize()
    _check("after the refused call", tr.adv.cpu().numpy(), tr.target.cpu().numpy(), p["value"], p["reward"], p["done"], p["tail"], cfg.gamma, cfg.lam, 0)
    ctx.close()


CRITIC_CASES = {
    "H64": dict(H=64, N=96),
    "H256-ragged": dict(H=256, N=100, oracle=True),
    "H96-padded": dict(H=96, N=70),
    "H384-wide": dict(H=384, N=70),
    "depth1": dict(H=64, N=96, depth=1),
    "depth3": dict(H=64, N=96, depth=3),
    "extra-critic-obs": dict(H=64, N=96, cfg=dict(extra_obs_critic=5)),
    "mirror": dict(H=64, N=96, cfg=dict(actor_mirror_loss_scale=1.0, critic_mirror_loss_scale=0.01)),
    "gemm-cell-layers": dict(H=64, N=96, env={"KBJ_ROLLOUT_STEP": "0"}),
}


@pytest.mark.parametrize("case", list(CRITIC_CASES))
def test_critic_value_is_the_policy_steps_value(case, monkeypatch):
    """kbj_critic_value = the value kbj_policy_step writes from the same carries and observation rows, bit for bit, and no carry moves."""
    import torch
    from kbot_joystick_amd.host import buffers
    c = CRITIC_CASES[case]
    H, N, depth, kw = c["H"], c["N"], c.get("depth", 2), c.get("cfg", {})
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)                  # read once, when the context is created
    m, cfg, ctx = _ctx(N, N, 4, H, depth=depth, gae_tail_value=1, **kw)
    mirror = "actor_mirror_loss_scale" in kw
    _, nc, lda, ldc = L.obs_widths(cfg)
    params = torch.zeros(ctx.param_count(), device="cuda:0")
    ctx.init_params(3, params)
    g = torch.Generator(device="cpu").manual_seed(11)
    aobs = torch.zeros(N, lda); aobs[:, :65] = torch.randn(N, 65, generator=g)
    cobs = torch.zeros(N, ldc); cobs[:, :nc] = torch.randn(N, nc, generator=g)
    aobs, cobs = aobs.cuda(), cobs.cuda()
    names = ["actor_hc", "critic_hc", "lpf"] + (["actor_mirror_hc", "critic_mirror_hc", "lpf_mirror"] if mirror else [])
    carry, twin = (buffers.CarryBuffers(N, H, depth, "cuda:0", mirror=mirror) for _ in range(2))
    for name in names:
        t = getattr(carry, name)
        t.copy_(torch.randn(t.shape, generator=g) * 0.5)
        getattr(twin, name).copy_(t)
    value = torch.full((N,), float("nan"), device="cuda:0")
    ctx.critic_value(params, cobs, carry.c, value)
    ctx.synchronize()
    for name in names:                            # nothing the caller owns moved
        assert torch.equal(getattr(carry, name), getattr(twin, name)), name
    action, logp, v_step = torch.zeros(N, L.NU, device="cuda:0"), torch.zeros(N, device="cuda:0"), torch.zeros(N, device="cuda:0")
    ctx.policy_step(params, aobs, cobs, twin.c, 7, 5, True, action, logp, v_step)
    ctx.synchronize()
    assert torch.isfinite(value).all() and float(value.abs().max()) > 1e-3
    assert torch.equal(value, v_step), float((value - v_step).abs().max())
    assert not torch.equal(twin.critic_hc, carry.critic_hc)          # the policy step did advance its copy
    value2 = torch.zeros_like(value)                                  # behind a policy step (the h planes are home again): the same answer
    ctx.critic_value(params, cobs, carry.c, value2)
    ctx.synchronize()
    assert torch.equal(value, value2)
    if c.get("oracle"):
        from oracle import nn as ON
        hc = carry.critic_hc.cpu().double()
        out_c, _ = ON.net_forward(ON.unflatten(params.cpu().double(), H), "critic", cobs[:, :475].cpu().double(), [[hc[l, 0], hc[l, 1]] for l in range(depth)])
        err = float((value.cpu().double() - out_c[:, 0]).abs().max())
        print(f"kbj_critic_value vs oracle at H = {H}, N = {N}: {err:.3g}")
        assert err < 2e-5
    ctx.close()


def test_critic_value_needs_the_switch():
    import torch
    from kbot_joystick_amd.host import binding as Bd, buffers
    m, cfg, ctx = _ctx(64, 64, 4, 64)
    params = torch.zeros(ctx.param_count(), device="cuda:0")
    carry = buffers.CarryBuffers(64, 64, 2, "cuda:0")
    with pytest.raises(Bd.KbjError, match="gae_tail_value"):
        ctx.critic_value(params, torch.zeros(64, L.LD_CRITIC, device="cuda:0"), carry.c, torch.zeros(64, device="cuda:0"))
    ctx.close()


def _task_cfg(**kw):
    from kbot_joystick_amd.host.task import launch_config
    base = dict(num_envs=64, batch_size=32, hidden_size=64, rollout_length_seconds=0.16, robot="kbot-headless", seed=4, num_passes=1, deterministic=True,
                termination_params={"episode_length": {"max_length_sec": 0.1}})       # 8 steps per rollout, episodes of at most 5: truncations in every rollout
    base.update(kw)
    return launch_config(**base)


def test_whole_task_with_both_switches():
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    cfg = _task_cfg(bootstrap_on_truncation=True, bootstrap_tail_value=True)
    fused = HumanoidWalkingTask(cfg)
    step = HumanoidWalkingTask(cfg, extra_terminations={"never": lambda state, level: torch.zeros(state.N, device="cuda")})
    assert (fused.kcfg.gae_bootstrap_truncation, fused.kcfg.gae_tail_value, fused.T, fused.kcfg.max_episode_steps) == (1, 1, 8, 5)
    for t in (fused, step):
        t.rollout()
    torch.cuda.synchronize()
    tail1 = fused.traj.value_tail.clone()
    assert torch.isfinite(tail1).all() and float(tail1.abs().max()) > 0 and torch.equal(tail1, step.traj.value_tail)
    # a second rollout without an update in between starts where the first one's tail pass looked: same row, same carries, same parameters, same launches
    for t in (fused, step):
        t.iteration += 1
        t.rollout()
    torch.cuda.synchronize()
    assert torch.equal(fused.traj.value[0], tail1)
    assert torch.equal(fused.traj.value_tail, step.traj.value_tail) and not torch.equal(fused.traj.value_tail, tail1)
    tr = fused.traj
    value, reward, done, tail = (x.cpu().numpy().copy() for x in (tr.value, tr.reward, tr.done, tr.value_tail))
    assert int((done > 0).sum()) >= 1 and int((done[-1] == 0).sum()) >= 1
    for t in (fused, step):
        t.update()                                   # GAE runs here, on the rollout's own arrays and the tail of the pre-update parameters
    torch.cuda.synchronize()
    _check("whole task", tr.adv.cpu().numpy(), tr.target.cpu().numpy(), value, reward, done, tail, fused.kcfg.gamma, fused.kcfg.lam, 1)
    base, _ = G.gae_ref(value, reward, done, fused.kcfg.gamma, fused.kcfg.lam)
    assert np.abs(tr.adv.cpu().numpy() - base).max() > 1e-3          # not the default conventions' answer
    assert torch.equal(tr.adv, step.traj.adv) and torch.equal(tr.target, step.traj.target)
    assert torch.equal(fused.params, step.params) and torch.isfinite(fused.params).all()
    for t in (fused, step):
        t.ctx.close()


def test_whole_task_with_both_switches_off_never_touches_the_tail(monkeypatch):
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    monkeypatch.delenv("KBJ_GAE_TRUNCATION", raising=False); monkeypatch.delenv("KBJ_GAE_TAIL", raising=False)
    task = HumanoidWalkingTask(_task_cfg())
    assert (task.kcfg.gae_bootstrap_truncation, task.kcfg.gae_tail_value) == (0, 0)
    task.traj.value_tail.fill_(float("nan"))
    task.train_iteration()
    torch.cuda.synchronize()
    assert bool(torch.isnan(task.traj.value_tail).all()) and torch.isfinite(task.traj.adv).all() and torch.isfinite(task.params).all()
    tr = task.traj
    _check("whole task, defaults", tr.adv.cpu().numpy(), tr.target.cpu().numpy(), tr.value.cpu().numpy(), tr.reward.cpu().numpy(), tr.done.cpu().numpy(), None,
           task.kcfg.gamma, task.kcfg.lam, 0)
    task.ctx.close()
