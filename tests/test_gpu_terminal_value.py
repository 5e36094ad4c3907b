"""The exact terminal value at time-outs on the GPU (kbj_config.gae_terminal_value; include/kbj.h kbj_env_step_terminal, kbj_critic_terminal_value,
kbj_set_terminal_values): the env kernels' terminal critic rows against a twin context without terminations, the sparse value kernel against
the oracle's critic in float64, the new row of kbj_gae against tests/gae_terminal_ref.py, the fused rollout against the ABI sequence issued by
hand, and the task facade. CPU halves (configs, references, liveness of the cases): tests/test_terminal_value_host.py."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import gae_ref as G
from tests import gae_terminal_ref as GT
from tests import helpers as H
from tests import terminal_value_cases as TV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _context(cfg, model=None):
    import torch
    from kbot_joystick_amd.host import binding as Bd
    model = model or compiler.load_model("kbot-headless")
    return Bd.Context(model, cfg, 0, torch.cuda.current_stream().cuda_stream)


def _done_ptr(aux_row):
    return aux_row.data_ptr() + 4 * L.AUX["DONE"]


# ---- env kernel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["newton", "cg"])
def test_env_step_terminal_rows(model, solver):
    """kbj_env_step_terminal from the fp32 oracle's states (N = 64, 10 steps, the case of the host emulation test): the terminal row of every env
    that ends = the next critic row of a twin context that steps the same state with terminations off, bit for bit on all columns; rows of envs
    that go on keep the sentinel; everything kbj_env_step writes is what kbj_env_step (a third context) writes from the same state."""
    import torch
    from oracle import oracle as O
    N, seed = TV.ENV_N, TV.ENV_SEED
    cfg, twin_cfg = TV.terminal_configs(N, int(solver == "newton"))
    term, plain, twin = _context(cfg, model), _context(cfg, model), _context(twin_cfg, model)
    o = O.Oracle(model, cfg, seed=seed, precision="f32")
    _, _, x0 = o.reset_all()
    rows = lambda: (torch.zeros(N, L.LD_ACTOR, device=DEV), torch.zeros(N, L.LD_CRITIC, device=DEV), torch.zeros(N, L.AUX["SIZE"], device=DEV))
    for c in (term, plain, twin):
        c.env_reset_all(seed, *rows())                # the contexts' seed; the states come from the oracle below
    rng = np.random.default_rng(0)
    counts = {1: 0, 2: 0, 3: 0}
    bits = lambda t: t.contiguous().view(torch.int32)
    for t in range(TV.ENV_STEPS):
        act = torch.from_numpy(np.ascontiguousarray(H.random_actions(model, rng, N), np.float32)).to(DEV)
        out = {}
        for name, c in (("term", term), ("plain", plain), ("twin", twin)):
            c.env_set_state(o.ep, o.es)
            aux_t, (a, cr, xn) = torch.from_numpy(x0).to(DEV), rows()
            if name == "term":
                ct = torch.full((N, L.LD_CRITIC), float(TV.SENTINEL), device=DEV)
                c.env_step_terminal(act, aux_t, a, cr, xn, ct)
            else:
                c.env_step(act, aux_t, a, cr, xn)
            ep, es = c.env_get_state()
            out[name] = dict(ep=torch.from_numpy(ep), es=torch.from_numpy(es), aux_t=aux_t.cpu(), actor=a.cpu(), critic=cr.cpu(), aux=xn.cpu())
        ct = ct.cpu()
        cause = TV.termination_causes(out["term"]["aux_t"].numpy(), cfg.unhealthy_z)
        for k in counts:
            counts[k] += int((cause == k).sum())
        ended = torch.from_numpy(cause != 0)
        assert bool((out["twin"]["aux_t"][:, L.AUX["DONE"]] == 0).all()), t
        assert torch.equal(bits(ct[ended]), bits(out["twin"]["critic"][ended])), (solver, t)
        assert bool((ct[~ended] == float(TV.SENTINEL)).all()), (solver, t)
        for k in ("ep", "es", "aux_t", "actor", "critic", "aux"):
            assert torch.equal(bits(out["term"][k]), bits(out["plain"][k])), (solver, t, k)
        aux = x0.copy()
        _, _, x0 = o.step(act.cpu().numpy(), aux)
    print(f"{solver}: terminal rows compared, by cause (height, tilt only, time-out): {counts}")
    assert all(v >= 1 for v in counts.values()), counts
    for c in (term, plain, twin):
        c.close()


def test_env_step_terminal_refuses_an_armed_state_record():
    import torch
    from kbot_joystick_amd.host import binding as Bd
    N = 64
    ctx = _context(L.default_config(num_envs=N, batch_size=N))
    a, c, x = torch.zeros(N, L.LD_ACTOR, device=DEV), torch.zeros(N, L.LD_CRITIC, device=DEV), torch.zeros(N, L.AUX["SIZE"], device=DEV)
    ctx.env_reset_all(1, a, c, x)
    act, ct, q = torch.zeros(N, L.NU, device=DEV), torch.zeros(N, L.LD_CRITIC, device=DEV), torch.zeros(N, L.QSTATE["SIZE"], device=DEV)
    ctx.call("kbj_env_record_state", q.data_ptr())
    with pytest.raises(Bd.KbjError, match="state record"):
        ctx.env_step_terminal(act, x.clone(), a.clone(), c.clone(), x.clone(), ct)
    ctx.env_step_terminal(act, x.clone(), a.clone(), c.clone(), x.clone(), ct)      # the record was disarmed: the context stays usable
    ctx.synchronize()
    ctx.close()


# ---- value kernel -------------------------------------------------------------------------------------------------------------------------
# native; zero padded to 128; the launch size; the wide schedule; and two sizes that are no multiple of 4, where the layers and the head take the
# scalar-load instantiations of the matrix-vector product (the others take the float4 ones)
VALUE_SHAPES = [(64, 1), (100, 2), (256, 2), (320, 1), (50, 1), (30, 2)]


@pytest.fixture(scope="module")
def value_problem():
    """`get(N, hidden_size, depth)`: _value_problem, computed once per shape for the module; the contexts are closed when the module is done."""
    cache = {}

    def get(N, Hs, depth):
        if (N, Hs, depth) not in cache:
            cache[(N, Hs, depth)] = _value_problem(N, Hs, depth)
        return cache[(N, Hs, depth)]
    yield get
    for p in cache.values():
        p["ctx"].close()


def _value_problem(N, Hs, depth, seed=11):
    """Random parameters from kbj_init_params, random finite carries and rows, the float64 oracle's critic on them, and what the existing full-width
    path (kbj_critic_value) misses that reference by. Returns a dict of device tensors and figures."""
    import torch
    from kbot_joystick_amd.host import buffers
    from oracle import nn as ON
    ctx = _context(L.default_config(num_envs=N, batch_size=N, rollout_len=4, hidden_size=Hs, depth=depth, gae_tail_value=1))
    params = torch.zeros(ctx.param_count(), device=DEV)
    ctx.init_params(3, params)
    g = torch.Generator(device="cpu").manual_seed(seed)
    rows = torch.zeros(N, L.LD_CRITIC); rows[:, :L.NOBS_CRITIC] = torch.randn(N, L.NOBS_CRITIC, generator=g)
    carry = buffers.CarryBuffers(N, Hs, depth, DEV)
    carry.critic_hc.copy_(torch.randn(carry.critic_hc.shape, generator=g) * 0.5)
    rows = rows.to(DEV)
    hc = carry.critic_hc.cpu().double()
    with torch.no_grad():
        ref, _ = ON.net_forward(ON.unflatten(params.cpu().double(), Hs, depth), "critic", rows[:, :L.NOBS_CRITIC].cpu().double(), [[hc[l, 0], hc[l, 1]] for l in range(depth)], depth)
    ref = ref[:, 0]
    full = torch.full((N,), float("nan"), device=DEV)
    ctx.critic_value(params, rows, carry.c, full)
    ctx.synchronize()
    err_full = float((full.cpu().double() - ref).abs().max())
    return dict(ctx=ctx, params=params, rows=rows, carry=carry, ref=ref, err_full=err_full, tol=4 * err_full)


@pytest.mark.parametrize("N", [70, 64])
@pytest.mark.parametrize("Hs,depth", VALUE_SHAPES)
def test_terminal_value_kernel(value_problem, N, Hs, depth):
    """kbj_critic_terminal_value against the oracle's critic in float64. Tolerance: 4 x what kbj_critic_value (the matrix-core path) misses the same
    reference by on the same inputs - the margin tests/test_gpu_deploy.py gives a vector-unit matrix-vector path, whose summation order differs.
    Measured (EXPERIMENTS.md "Terminal value"): see the table there."""
    import torch
    p = value_problem(N, Hs, depth)
    ctx, params, rows, carry, ref, tol = p["ctx"], p["params"], p["rows"], p["carry"], p["ref"], p["tol"]
    assert 0 < p["err_full"] < 1e-4 and float(ref.abs().max()) > 1e-2
    hc0, rows0 = carry.critic_hc.clone(), rows.clone()
    g = torch.Generator(device="cpu").manual_seed(5)
    sign = torch.randint(-1, 2, (N,), generator=g).float()
    sign[:3] = torch.tensor([-1.0, 0.0, 1.0])
    patterns = {"none positive": torch.where(sign > 0, torch.zeros(N), sign), "all positive": torch.ones(N), "mixed": sign}
    worst = 0.0
    for name, done in patterns.items():
        pos = done > 0
        value = torch.full((N,), float("nan"), device=DEV)
        if name == "mixed":       # the DONE column of an aux record (-1 rows included); rows that are not valued may hold anything: they are not read
            aux = torch.full((N, L.AUX["SIZE"]), float("nan"), device=DEV)
            aux[:, L.AUX["DONE"]] = done.to(DEV)
            r = rows.clone(); r[~pos.to(DEV)] = float("nan")
            ctx.critic_terminal_value(params, r, carry.c, _done_ptr(aux), L.AUX["SIZE"], value)
        else:
            d = done.to(DEV)
            ctx.critic_terminal_value(params, rows, carry.c, d, 1, value)
        ctx.synchronize()
        v = value.cpu()
        assert bool((v[~pos].view(torch.int32) == 0).all()), name           # exactly +0.0f where nothing timed out
        if pos.any():
            err = float((v[pos].double() - ref[pos]).abs().max())
            worst = max(worst, err)
            assert err <= tol, (name, err, tol)
        assert int(pos.sum()) == (0 if name == "none positive" else N if name == "all positive" else int((sign > 0).sum()))
        assert torch.equal(carry.critic_hc, hc0) and torch.equal(rows, rows0), name   # read only
    print(f"terminal value N = {N}, H = {Hs}, depth = {depth}: max |err| vs float64 {worst:.3g}; kbj_critic_value {p['err_full']:.3g}; bound {tol:.3g}")


# ---- GAE ----------------------------------------------------------------------------------------------------------------------------------
def _gae_setup(N, T, **kw):
    import torch
    from kbot_joystick_amd.host import buffers
    p = TV.terminal_problem(N, T)
    ctx = _context(L.default_config(num_envs=N, batch_size=N, rollout_len=T, hidden_size=64, depth=1, gae_bootstrap_truncation=1, gae_terminal_value=1, **kw))
    tr = buffers.TrajBuffers(T, N, 64, 1, DEV, terminal_value=True)
    tr.aux[:T, :, L.AUX["DONE"]] = torch.from_numpy(p["done"]).to(DEV)
    tr.reward.copy_(torch.from_numpy(p["reward"])); tr.value.copy_(torch.from_numpy(p["value"])); tr.value_tail.copy_(torch.from_numpy(p["tail"]))
    tr.value_term.copy_(torch.from_numpy(p["value_term"]))
    return p, ctx, tr


@pytest.mark.parametrize("tail_on", [0, 1])
def test_gae_terminal_row(tail_on):
    """N = 64, T = 8, all three signs of DONE (the last row too): kbj_gae against tests/gae_terminal_ref.py within the fp32 bound
    tests/test_gpu_gae_boundary.py derives for its siblings (gae_ref.gae_bound, the terminal values among the bootstrap operands)."""
    import torch
    N, T = 64, 8
    p, ctx, tr = _gae_setup(N, T, gae_tail_value=tail_on)
    last = p["done"][-1]
    assert (last > 0).sum() >= 1 and (last < 0).sum() >= 1 and (last == 0).sum() >= 1
    ctx.set_terminal_values(tr.value_term)
    tr.adv.fill_(float("nan")); tr.target.fill_(float("nan"))
    ctx.gae(tr.c, tr.adv, tr.target)
    ctx.synchronize()
    cfg = ctx.config
    tail = p["tail"] if tail_on else None
    adv, tgt = GT.gae_terminal_ref(p["value"], p["reward"], p["done"], cfg.gamma, cfg.lam, p["value_term"], tail)
    bound = GT.gae_terminal_bound(p["value"], p["reward"], tail, p["value_term"], adv, cfg.gamma, cfg.lam)
    ea, et = np.abs(tr.adv.cpu().numpy().astype(np.float64) - adv).max(), np.abs(tr.target.cpu().numpy().astype(np.float64) - tgt).max()
    trunc, _ = G.gae_ref(p["value"], p["reward"], p["done"], cfg.gamma, cfg.lam, 1, tail)
    print(f"gae terminal row, tail {tail_on}: adv err {ea:.3g}, target err {et:.3g}, bound {bound:.3g}; the switch moves adv by {np.abs(adv - trunc).max():.3g}")
    assert ea <= bound and et <= bound, (ea, et, bound)
    assert np.abs(adv - trunc).max() >= 100 * bound      # a kernel that ignored the switch could not pass
    ctx.close()


def test_terminal_switch_without_the_buffer_is_an_error():
    import torch
    from kbot_joystick_amd.host import binding as Bd, buffers
    N, T = 64, 8
    p, ctx, tr = _gae_setup(N, T)
    tr.adv.fill_(7.0)
    with pytest.raises(Bd.KbjError, match="kbj_set_terminal_values"):
        ctx.gae(tr.c, tr.adv, tr.target)
    params = torch.zeros(ctx.param_count(), device=DEV)
    ctx.init_params(3, params)
    carry = buffers.CarryBuffers(N, 64, 1, DEV)
    ctx.env_reset_all(3, tr.actor_obs[T], tr.critic_obs[T], tr.aux[T])
    tr.action.fill_(7.0)
    with pytest.raises(Bd.KbjError, match="kbj_set_terminal_values"):
        ctx.rollout(params, carry.c, 3, 0, tr.c)
    ctx.synchronize()
    assert bool((tr.adv == 7.0).all()) and bool((tr.action == 7.0).all())      # nothing was launched
    ctx.set_terminal_values(tr.value_term)                                      # the context stays usable
    ctx.gae(tr.c, tr.adv, tr.target)
    ctx.rollout(params, carry.c, 3, 0, tr.c)
    ctx.synchronize()
    assert torch.isfinite(tr.adv).all() and torch.isfinite(tr.action).all() and torch.isfinite(tr.value_term).all()
    ctx.set_terminal_values(None)
    with pytest.raises(Bd.KbjError, match="kbj_set_terminal_values"):
        ctx.gae(tr.c, tr.adv, tr.target)
    ctx.close()


# ---- fused rollout against the ABI sequence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [5, 1, 2])
def test_fused_rollout_against_the_abi_sequence(m):
    """N = 64, T = 8, episodes of at most m steps, H = 64, depth 1: every env times out inside the rollout, all on the same step(s). The [T][N]
    terminal values of kbj_rollout = those of (kbj_policy_step, kbj_env_step_terminal, kbj_critic_terminal_value, kbj_carry_reset) issued by hand,
    bit for bit; the rest of the trajectory = the same rollout with the switch off, bit for bit. m = 1 and 2: every env ends again one or two
    steps later, so the env step rewrites every row of the ONE terminal scratch while the critic's lane may still owe the previous step's
    values - what the plan's ev_term orders (the serial by-hand sequence is the reference that cannot go wrong there)."""
    import torch
    from kbot_joystick_amd.host import buffers
    N, T, Hs, seed = 64, 8, 64, 4
    base = dict(num_envs=N, batch_size=N, rollout_len=T, hidden_size=Hs, depth=1, max_episode_steps=m, gae_bootstrap_truncation=1)
    runs = {}
    for name, term in (("fused", 1), ("by hand", 1), ("off", 0)):
        ctx = _context(L.default_config(gae_terminal_value=term, **base))
        tr, carry = buffers.TrajBuffers(T, N, Hs, 1, DEV, terminal_value=True), buffers.CarryBuffers(N, Hs, 1, DEV)
        tr.value_term.fill_(float("nan"))
        params = torch.zeros(ctx.param_count(), device=DEV)
        ctx.init_params(seed, params)
        ctx.env_reset_all(seed, tr.actor_obs[T], tr.critic_obs[T], tr.aux[T])
        if term:
            ctx.set_terminal_values(tr.value_term)
        if name == "by hand":
            tr.actor_obs[0].copy_(tr.actor_obs[T]); tr.critic_obs[0].copy_(tr.critic_obs[T]); tr.aux[0].copy_(tr.aux[T])
            for t in range(T):
                ctx.policy_step(params, tr.actor_obs[t], tr.critic_obs[t], carry.c, seed, t, False, tr.action[t], tr.logp[t], tr.value[t])
                ctx.env_step_terminal(tr.action[t], tr.aux[t], tr.actor_obs[t + 1], tr.critic_obs[t + 1], tr.aux[t + 1], tr.term_rows)
                ctx.critic_terminal_value(params, tr.term_rows, carry.c, _done_ptr(tr.aux[t]), L.AUX["SIZE"], tr.value_term[t])
                ctx.carry_reset(carry.c, _done_ptr(tr.aux[t]), L.AUX["SIZE"])
            ctx.rewards(tr.aux, T, tr.reward, tr.comps)
        else:
            ctx.rollout(params, carry.c, seed, 0, tr.c)
        ctx.synchronize()
        runs[name] = (ctx, tr, carry)
    fused, hand, off = (runs[k][1] for k in ("fused", "by hand", "off"))
    done = fused.done
    assert bool((done[m - 1::m] > 0).all()) and int((done > 0).sum()) == N * (T // m), "every env times out on every m-th control step, and nowhere else"
    vt = fused.value_term
    assert torch.isfinite(vt).all() and bool((vt[done <= 0] == 0).all()) and float(vt[m - 1].abs().min()) > 0
    assert not torch.equal(vt[m - 1], fused.value[m - 1])              # not V(s_t), the stand-in
    assert torch.equal(vt.view(torch.int32), hand.value_term.view(torch.int32))
    assert bool(torch.isnan(off.value_term).all())                      # the switch off: never touched
    for k in ("actor_obs", "critic_obs", "aux", "action", "logp", "value", "reward"):
        assert torch.equal(getattr(fused, k), getattr(off, k)), k
        assert torch.equal(getattr(fused, k), getattr(hand, k)), k
    for k in ("actor_hc", "critic_hc", "lpf"):
        assert torch.equal(getattr(runs["fused"][2], k), getattr(runs["off"][2], k)), k
    for ctx, _, _ in runs.values():
        ctx.close()


# ---- task facade ----------------------------------------------------------------------------------------------------------------------------
def _task_cfg(**kw):
    from kbot_joystick_amd.host.task import launch_config
    base = dict(num_envs=64, batch_size=32, hidden_size=64, rollout_length_seconds=0.16, robot="kbot-headless", seed=4, num_passes=1, deterministic=True,
                termination_params={"episode_length": {"max_length_sec": 0.1}})       # 8 steps per rollout, episodes of at most 5: the shape of test_gpu_gae_boundary.py's task test
    base.update(kw)
    return launch_config(**base)


class _TimeOutTerm:
    """A user Termination term that restates the time-out: +1 on the `steps`-th control step of an env's episode."""

    def __init__(self, steps):
        self.steps, self.count = steps, None

    def __call__(self, state, level):
        import torch
        if self.count is None:
            self.count = torch.zeros(state.N, device=state.done.device)
        self.count += 1
        fire = (self.count >= self.steps) & (state.done == 0)
        self.count = torch.where(fire | (state.done != 0), torch.zeros_like(self.count), self.count)
        return fire.float()


def test_task_with_the_terminal_value(value_problem):
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    on = dict(bootstrap_on_truncation=True, bootstrap_terminal_value=True)
    with pytest.raises(ValueError, match="extra_critic_obs") as e:
        HumanoidWalkingTask(_task_cfg(extra_critic_obs=3, **on))
    assert "bootstrap_terminal_value" in str(e.value)
    term, trunc = HumanoidWalkingTask(_task_cfg(**on)), HumanoidWalkingTask(_task_cfg(bootstrap_on_truncation=True))
    user = HumanoidWalkingTask(_task_cfg(termination_params={"episode_length": {"max_length_sec": float("inf")}}, **on), extra_terminations={"time_out": _TimeOutTerm(5)})
    assert (term.kcfg.gae_bootstrap_truncation, term.kcfg.gae_terminal_value, term.T, term.kcfg.max_episode_steps) == (1, 1, 8, 5)
    assert trunc.kcfg.gae_terminal_value == 0 and trunc.traj.value_term is None and user.kcfg.max_episode_steps == 2 ** 30
    for t in (term, trunc, user):
        t.rollout()
    torch.cuda.synchronize()
    done = term.traj.done.cpu().numpy()
    assert int((done > 0).sum()) >= 32
    for k in ("critic_obs", "aux", "action", "value", "reward"):
        assert torch.equal(getattr(term.traj, k), getattr(trunc.traj, k)), k
    # the user term's +1 on the step-wise path (the pre-reset critic row copied into the terminal scratch) gives what the built-in time-out gives fused
    assert torch.equal(user.traj.done, term.traj.done)
    tol = value_problem(64, 64, 2)["tol"]
    vt, vu = term.traj.value_term, user.traj.value_term
    pos = term.traj.done > 0
    diff = float((vt - vu).abs().max())
    print(f"terminal values, fused built-in time-out vs step-wise user term: max difference {diff:.3g} (tolerance {tol:.3g})")
    assert diff <= tol and bool((vu[~pos] == 0).all()) and float(vt[pos].abs().min()) > 0
    value, reward, vterm = (x.cpu().numpy().copy() for x in (term.traj.value, term.traj.reward, vt))
    for t in (term, trunc):
        t.update()                                   # one update runs; GAE on the rollout's own arrays
    torch.cuda.synchronize()
    assert torch.isfinite(term.params).all() and torch.isfinite(term.metrics).all()
    g, l = term.kcfg.gamma, term.kcfg.lam
    adv, _ = GT.gae_terminal_ref(value, reward, done, g, l, vterm)
    bound = GT.gae_terminal_bound(value, reward, None, vterm, adv, g, l)
    assert np.abs(term.traj.adv.cpu().numpy() - adv).max() <= bound
    # against the bootstrap_on_truncation-only run: the time-out rows and the rows that chain into them, and nothing else
    moved = (term.traj.adv != trunc.traj.adv).cpu().numpy()
    assert np.array_equal(moved, GT.affected_rows(done)), (int(moved.sum()), int(GT.affected_rows(done).sum()))
    for t in (term, trunc, user):
        t.close()
