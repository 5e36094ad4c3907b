"""kbj_deploy_init / kbj_deploy_step (convert.py init_fn / step_fn, csrc/kbj_deploy.h) on the GPU, through ctypes, against tests/deploy_ref.py
in float64.

Accuracy has no fixed tolerance: the yardstick is the parent's only way to step a policy, kbj_policy_step(argmax=1), given the same rows
(packed in float64, rounded to float32) on a context with num_envs = N and measured against the same reference in the same run. The new
path may err at most 4x the yardstick's largest error per quantity (action, h, c), with a floor of 2^-22 max|value| for steps where the
yardstick happens to be exact: both sum the same 65..1024-term products in fp32 in a different order and use the same hardware exp / rcp,
so a larger factor is an arithmetic difference, not rounding. Everything else is demanded bit for bit.

Measured on an MI355X, largest error over 8 chained steps against the float64 chain, deployed step / kbj_policy_step(argmax=1) (the bound
is 4x the second figure; the whole table with h, c and the bounds: EXPERIMENTS.md, "Deployed actor step"):
  (H, depth, N)   action               c
  (256, 2, 1)     1.97e-7 / 5.00e-7    5.00e-7 / 1.43e-6
  (256, 2, 5)     2.59e-7 / 4.32e-7    5.32e-7 / 1.35e-6
  (128, 2, 3)     3.01e-7 / 5.02e-7    4.11e-7 / 9.48e-7
  (64, 1, 2)      2.08e-7 / 2.57e-7    3.87e-7 / 9.63e-7
  (90, 3, 2)      2.85e-7 / 2.96e-7    3.74e-7 / 5.75e-7
  (512, 4, 2)     3.27e-7 / 4.49e-7    6.45e-7 / 1.74e-6
  teacher-forced rollout (4 envs, T = 8, H = 128): 3.03e-7 / 4.28e-7 on the action."""
import ctypes as C
import functools

import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import deploy_ref as DR

pytestmark = pytest.mark.gpu

CASES = [(256, 2, 1), (256, 2, 5), (128, 2, 3), (64, 1, 2), (90, 3, 2), (512, 4, 2)]   # (90, 3, 2): scalar loads, a size the training path pads; (512, 4, 2): the largest served
STEPS, GUARD, SENTINEL = 8, 64, 1.2345e30


class Guarded:
    """A device array inside two bands of GUARD sentinel floats; the payload starts sentinel-filled too."""

    def __init__(self, torch, *shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, device="cuda:0")
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _params(H, depth, seed=11, scale=3.0):
    """kbj_init_params' vector as tests/helpers.init_params_ref restates it (the same leaves, numbered and laid out the same way, from
    init_uniform_ref), scaled so the gates leave the linear region: float32. Only the actor's leaves are drawn - the critic's half of the
    threefry stream is most of the time at H = 512 and nothing here reads it - the critic's stay zero."""
    from oracle import nn as ON
    from tests import helpers
    flat, off = np.zeros(sum(L.param_count(H, depth)), np.float32), 0
    for leaf, (name, shp) in enumerate(ON.param_shapes(H, depth)):
        n = int(np.prod(shp))
        if name.startswith("actor."):
            flat[off:off + n] = helpers.init_uniform_ref(seed, leaf, n, ON.NOBS_ACTOR if ".input_proj." in name else H)
        off += n
    return flat * np.float32(scale)


def _sensor_steps(model, N, seed):
    """STEPS seeded sensor sets; the first two (step, row) slots hold commands on either side of the zero-command threshold, neither on it."""
    gen = np.random.default_rng(seed)
    steps = [DR.random_sensors(model, gen, N) for _ in range(STEPS)]
    for k, (norm, axis) in enumerate(((0.9e-3, 0), (1.1e-3, 2))):
        cmd = steps[k // N][4]
        cmd[k % N, :3] = 0
        cmd[k % N, axis] = norm
    assert all(np.abs(s[4][:, 6:]).min() > 0 for s in steps)             # arm commands are non-zero
    return steps


def _dev(torch, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


@functools.lru_cache(maxsize=None)
def _run(H, depth, N):
    """One case, every variant, computed once: the float64 reference chain, the deployed chain (out of place, guarded), the same chain in
    place, every row alone with N = 1, the last call repeated, the actor prefix / a 4-byte shifted copy of the parameters, and the yardstick."""
    import torch
    from kbot_joystick_amd.host import binding as Bd, buffers, deploy
    model = compiler.load_model("kbot-headless")
    cfg = L.default_config(num_envs=N, batch_size=N, rollout_len=4, hidden_size=H, depth=depth)
    ctx = Bd.Context(model, cfg, 0, torch.cuda.current_stream().cuda_stream)
    cs, alpha = ctx.deploy_carry_size(), float(cfg.lpf_alpha)
    assert cs == DR.carry_size(H, depth)
    pn = _params(H, depth)
    params = torch.from_numpy(pn).to("cuda:0")
    na = ctx.actor_param_count()
    steps = _sensor_steps(model, N, 100 * H + N)
    out = dict(H=H, depth=depth, N=N)

    # float64 reference chain
    leaves = DR.actor_leaves(pn, H, depth)
    ref_carry, ref = DR.init(N, H, depth), []
    for s in steps:
        a, ref_carry = DR.step(leaves, model, alpha, H, depth, *s, ref_carry)
        ref.append((a, ref_carry))

    # kbj_deploy_init: zeros and nothing else
    g0 = Guarded(torch, N, cs)
    ctx.deploy_init(N, g0.t)
    ctx.synchronize()
    out["init_zero"], out["init_guards"] = bool((g0.t == 0).all()), g0.intact()

    # the chain out of place (ping-pong between two guarded carries), guarded action
    ga, gc = Guarded(torch, N, 20), [g0, Guarded(torch, N, cs)]
    inplace = torch.zeros(N, cs, device="cuda:0")
    a_ip = torch.zeros(N, 20, device="cuda:0")
    chain, carries_in, ok = [], [], dict(guards=True, tail=True, inplace=True, alone=True)
    for t, s in enumerate(steps):
        d = _dev(torch, s)
        cin, cout = gc[t % 2], gc[(t + 1) % 2]
        carries_in.append(cin.t.clone())
        ctx.deploy_step(params, *d, N, cin.t, cout.t, ga.t)
        ctx.deploy_step(params, *d, N, inplace, inplace, a_ip)
        ctx.synchronize()
        ok["guards"] &= ga.intact() and cin.intact() and cout.intact()
        ok["tail"] &= torch.equal(cout.t[:, -20:], ga.t)
        ok["inplace"] &= torch.equal(inplace, cout.t) and torch.equal(a_ip, ga.t)
        for r in range(N):                                     # row r stepped alone
            c1, a1 = carries_in[t][r:r + 1].clone(), torch.zeros(1, 20, device="cuda:0")
            ctx.deploy_step(params, *[x[r:r + 1].contiguous() for x in d], 1, c1, c1, a1)
            ok["alone"] &= torch.equal(c1[0], cout.t[r]) and torch.equal(a1[0], ga.t[r])
        chain.append((ga.t.cpu().numpy().copy(), cout.t.cpu().numpy().copy()))
    out.update(ok)

    # the last call again, with the actor's prefix alone, and with a copy of the parameters that is not 16-byte aligned
    d, cin = _dev(torch, steps[-1]), carries_in[-1]
    variants = {}
    shifted = torch.zeros(pn.size + 1, device="cuda:0")
    shifted[1:].copy_(params)
    for name, p in (("twice", params), ("prefix", params[:na].clone()), ("unaligned", shifted[1:])):
        a2, c2 = Guarded(torch, N, 20), Guarded(torch, N, cs)
        ctx.deploy_step(p, *d, N, cin, c2.t, a2.t)
        ctx.synchronize()
        variants[name] = torch.equal(a2.t, ga.t) and torch.equal(c2.t, gc[STEPS % 2].t) and a2.intact() and c2.intact()
    out["variants"] = variants

    # the yardstick: kbj_policy_step(argmax = 1) on the same rows packed in float64 and rounded to fp32
    carry = buffers.CarryBuffers(N, H, depth, "cuda:0")
    action, logp, value = torch.zeros(N, 20, device="cuda:0"), torch.zeros(N, device="cuda:0"), torch.zeros(N, device="cuda:0")
    cobs = torch.zeros(N, L.LD_CRITIC, device="cuda:0")
    yard = []
    for t, s in enumerate(steps):
        aobs = torch.zeros(N, L.LD_ACTOR)
        aobs[:, :65] = torch.from_numpy(DR.pack(model, *s).astype(np.float32))
        ctx.policy_step(params, aobs.cuda(), cobs, carry.c, 7, t, True, action, logp, value)
        ctx.synchronize()
        yard.append((action.cpu().numpy().copy(), deploy.flat_carry_from(carry).cpu().numpy()))
    ctx.close()

    def errors(path):
        e = dict(action=0.0, h=0.0, c=0.0)
        for (a, c), (ra, rc) in zip(path, ref):
            hc, rhc = c[:, :-20].reshape(N, depth, 2, H), rc[:, :-20].reshape(N, depth, 2, H)
            e["action"] = max(e["action"], float(np.abs(a - ra).max()))
            e["h"] = max(e["h"], float(np.abs(hc[:, :, 0] - rhc[:, :, 0]).max()))
            e["c"] = max(e["c"], float(np.abs(hc[:, :, 1] - rhc[:, :, 1]).max()))
        return e
    out["err"], out["yard"] = errors(chain), errors(yard)
    rhc = np.stack([rc[:, :-20].reshape(N, depth, 2, H) for _, rc in ref])
    out["scale"] = dict(action=max(float(np.abs(a).max()) for a, _ in ref), h=float(np.abs(rhc[:, :, :, 0]).max()), c=float(np.abs(rhc[:, :, :, 1]).max()))
    out["finite"] = all(np.isfinite(a).all() and np.isfinite(c).all() for a, c in chain)
    return out


@pytest.mark.parametrize("H,depth,N", CASES)
def test_deployed_step_is_as_accurate_as_the_policy_step(H, depth, N):
    r = _run(H, depth, N)
    assert r["finite"] and r["scale"]["c"] > 0.5            # the recurrence has left the linear region
    lines = []
    for q in ("action", "h", "c"):
        bound = max(4 * r["yard"][q], 2.0 ** -22 * r["scale"][q])
        lines.append((q, r["err"][q], r["yard"][q], bound))
        print(f"deploy H={H} depth={depth} N={N} {q:6s}: deployed {r['err'][q]:.3e}  policy_step {r['yard'][q]:.3e}  bound {bound:.3e}  max|value| {r['scale'][q]:.3f}")
    for q, e, y, bound in lines:
        assert e <= bound, (q, e, y, bound)


@pytest.mark.parametrize("H,depth,N", CASES)
def test_deployed_step_bit_for_bit_demands(H, depth, N):
    r = _run(H, depth, N)
    assert r["init_zero"] and r["init_guards"], "kbj_deploy_init writes zeros and nothing else"
    assert r["tail"], "the last 20 floats of carry_out are the action"
    assert r["alone"], "row r of an N-row call equals the row stepped alone with N = 1"
    assert r["inplace"], "in-place and out-of-place carry give the same bits"
    assert r["variants"]["twice"], "the same call twice gives the same bits"
    assert r["guards"], "guard bands are untouched"
    assert r["variants"]["prefix"], "a full params_d and its actor prefix give the same bits"
    assert r["variants"]["unaligned"], "vector and scalar loads of the parameters give the same bits"


def test_teacher_forced_against_a_real_rollout():
    """4 envs, kbj_rollout acting with the mode, T = 8, H = 128: at every step the deployed actor is fed sensors_from_actor_obs of the
    rollout's own observation row and must return the rollout's action - under the same 4x rule, both measured against deploy_ref on
    those sensors - with its flat carry rows zeroed where the step ended an episode, as kbj_carry_reset does."""
    import torch
    from kbot_joystick_amd.host import binding as Bd, buffers, deploy
    N, T, H, depth, seed = 4, 8, 128, 2, 3
    model = compiler.load_model("kbot-headless")
    cfg = L.default_config(num_envs=N, batch_size=N, rollout_len=T, hidden_size=H, depth=depth)
    ctx = Bd.Context(model, cfg, 0, torch.cuda.current_stream().cuda_stream)
    params = torch.zeros(ctx.param_count(), device="cuda:0")
    ctx.init_params(seed, params)
    params *= 3.0
    tr, carry = buffers.TrajBuffers(T, N, H, depth, "cuda:0"), buffers.CarryBuffers(N, H, depth, "cuda:0")
    ctx.env_reset_all(seed, tr.actor_obs[T], tr.critic_obs[T], tr.aux[T])
    ctx.set_rollout_argmax(True)
    ctx.rollout(params, carry.c, seed, 0, tr.c)
    ctx.synchronize()
    pn, alpha = params.cpu().numpy(), float(cfg.lpf_alpha)
    leaves = DR.actor_leaves(pn, H, depth)
    flat, ref_carry = torch.zeros(N, ctx.deploy_carry_size(), device="cuda:0"), DR.init(N, H, depth)
    ctx.deploy_init(N, flat)
    action = torch.zeros(N, 20, device="cuda:0")
    e_dep = e_roll = scale = 0.0
    for t in range(T):
        sens = deploy.sensors_from_actor_obs(tr.actor_obs[t], model)
        ctx.deploy_step(params, *sens, N, flat, flat, action)
        ctx.synchronize()
        ra, ref_carry = DR.step(leaves, model, alpha, H, depth, *[s.cpu().numpy() for s in sens], ref_carry)
        e_dep = max(e_dep, float(np.abs(action.cpu().numpy() - ra).max()))
        e_roll = max(e_roll, float(np.abs(tr.action[t].cpu().numpy() - ra).max()))
        scale = max(scale, float(np.abs(ra).max()))
        done = tr.aux[t, :, L.AUX["DONE"]] != 0
        flat[done] = 0.0
        ref_carry[done.cpu().numpy()] = 0.0
    ctx.synchronize()
    hc, lpf = deploy.carry_from_flat(flat, depth, H)
    bound = max(4 * e_roll, 2.0 ** -22 * scale)
    print(f"teacher-forced rollout: deployed {e_dep:.3e}  rollout {e_roll:.3e}  bound {bound:.3e}  max|action| {scale:.3f}  "
          f"final carry vs rollout: hc {float((hc - carry.actor_hc).abs().max()):.3e} lpf {float((lpf - carry.lpf).abs().max()):.3e}")
    ctx.close()
    assert scale > 0.1 and e_dep <= bound, (e_dep, e_roll, bound)


def test_archive_and_live_parameters_agree_bit_for_bit(tmp_path):
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    from tests.test_gpu_host import _small
    task = HumanoidWalkingTask(_small(num_envs=8, batch_size=8))
    path = str(tmp_path / "actor.npz")
    task.export_actor(path)
    archived, live = task.deployed_actor(path), task.deployed_actor()
    n = 3
    sens = _dev(torch, DR.random_sensors(task.model_blob, np.random.default_rng(0), n))
    ca, cl = archived.init(n), live.init(n)
    assert ca.shape == (n, task.kcfg.depth * 2 * task.H + 20) and torch.equal(ca, cl) and bool((ca == 0).all())
    (aa, ca2), (al, cl2) = archived.step(*sens, ca), live.step(*sens, cl)
    torch.cuda.synchronize()
    assert torch.equal(aa, al) and torch.equal(ca2, cl2) and bool(aa.abs().max() > 0)
    a1, c1 = live.step(*[s[0] for s in sens], cl[0])          # one row without the batch dimension
    torch.cuda.synchronize()
    assert a1.shape == (20,) and torch.equal(a1, al[0]) and torch.equal(c1, cl2[0])
    archived.close()
    task.ctx.close()


def test_refusals_launch_nothing():
    import torch
    from kbot_joystick_amd.host import binding as Bd
    model = compiler.load_model("kbot-headless")
    N, H = 2, 64

    def attempt(ctx, n):
        cs = ctx.deploy_carry_size()
        params = torch.zeros(ctx.param_count(), device="cuda:0")
        sens = _dev(torch, DR.random_sensors(model, np.random.default_rng(0), N))
        carry, action = Guarded(torch, N, cs), Guarded(torch, N, 20)
        inp = Bd.DeployInputs(*[s.data_ptr() for s in sens])
        rc = ctx.lib.kbj_deploy_step(ctx._h, params.data_ptr(), C.byref(inp), n, carry.t.data_ptr(), carry.t.data_ptr(), action.t.data_ptr())
        msg = ctx.lib.kbj_last_error(ctx._h).decode()
        ctx.synchronize()
        untouched = bool((carry.buf == SENTINEL).all()) and bool((action.buf == SENTINEL).all())
        return rc, msg, untouched

    ctx = Bd.Context(model, L.default_config(num_envs=N, batch_size=N, hidden_size=H, extra_obs_actor=4), 0, torch.cuda.current_stream().cuda_stream)
    rc, msg, untouched = attempt(ctx, N)
    ctx.close()
    assert rc != 0 and "extra_obs_actor" in msg and untouched
    ctx = Bd.Context(model, L.default_config(num_envs=N, batch_size=N, hidden_size=H), 0, torch.cuda.current_stream().cuda_stream)
    rc, msg, untouched = attempt(ctx, 0)
    assert rc != 0 and "N must be positive" in msg and untouched
    with pytest.raises(Bd.KbjError, match="N must be positive"):
        ctx.deploy_init(0, torch.zeros(4, device="cuda:0"))
    with pytest.raises(Bd.KbjError, match="null"):
        ctx.deploy_init(1, None)
    ctx.close()
