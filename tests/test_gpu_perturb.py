"""kbj_env_perturb on the GPU: the rows it writes against tests/robustness_ref.py perturbed_row, bit for bit; what it must leave alone; its
refusals; and the step kernel under the rows it wrote, teacher-forced against the oracle (the loop of
tests/test_gpu_push.py::test_scripted_push_matches_the_oracle).

Bounds. Rows, status and everything left alone: bit for bit. Dynamics: tests/helpers.TOL, unchanged. The fp32 oracle against the fp64 one on
exactly these env-steps sits inside that table (measured on the CPU, tests/test_robustness_host.py prints them: qpos 1.8e-7 / 8.4e-7 /
4.9e-3 against 4e-7 / 2e-6 / 0.1; qvel 7.8e-7 / 3.7e-6 / 0.17 against 1.5e-6 / 1e-5 / 1.0; qacc 3.1e-6 / 2.0e-5 / 0.92 against 6e-6 /
4e-5 / 4.0, median / p99 / max; the one large value sits on the torque x 0.5 case, at a clip edge), and so does the host emulation of the
kernel body. No env-step of the setup ends an episode on the oracle, so none may be left out."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import helpers as H
from tests import robustness_ref as RR

pytestmark = pytest.mark.gpu
EP, P = L.EP, L.PERT
N_ROWS = 70           # one full wavefront's worth of envs and a remainder


def _ctx(model, cfg):
    import torch
    from kbot_joystick_amd.host import binding as B
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return B.Context(model, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream), torch


def _obs(torch, N):
    dev = "cuda:0"
    return (torch.zeros(N, L.LD_ACTOR, device=dev), torch.zeros(N, L.LD_CRITIC, device=dev), torch.zeros(N, L.AUX["SIZE"], device=dev))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _records(rng, n):
    """Valid records that turn every knob, per joint too; LATENCY negative (whole and not), and 0 .. 5; the spare words hold anything."""
    r = np.zeros((n, P["SIZE"]), np.float32)
    r[:, P["MASS_SCALE"]] = rng.uniform(0.7, 1.3, n)
    r[:, P["PAYLOAD"]] = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0, 8, n))
    r[:, P["MU_SCALE"]] = rng.uniform(0.25, 1.5, n)
    r[:, P["ARMATURE_SCALE"]] = rng.uniform(0.5, 2.0, n)
    r[:, P["FRICLOSS_SCALE"]] = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0, 3, n))
    r[:, P["LATENCY"]] = rng.choice(np.array([-1, -0.5, -3, 0, 1, 2, 3, 4, 5], np.float32), n)
    r[:, P["COM_SHIFT"]:P["COM_SHIFT"] + 3] = rng.uniform(-0.05, 0.05, (n, 3))
    r[:, P["SPARE"]:P["KP_SCALE"]] = rng.choice(np.array([0, np.nan, np.inf, -7], np.float32), (n, 3))
    r[:, P["KP_SCALE"]:P["KD_SCALE"]] = rng.uniform(0.5, 1.5, (n, L.NU))
    r[:, P["KD_SCALE"]:P["TAULIM_SCALE"]] = np.where(rng.random((n, L.NU)) < 0.1, 0.0, rng.uniform(0, 1.5, (n, L.NU)))
    r[:, P["TAULIM_SCALE"]:P["ACTBIAS"]] = rng.uniform(0.4, 1.0, (n, L.NU))
    r[:, P["ACTBIAS"]:] = rng.uniform(-0.05, 0.05, (n, L.NU))
    assert all(RR.record_valid(x) for x in r)
    return r


def _perturb(ctx, torch, mask, recs, with_status=True):
    status = torch.full((recs.shape[0],), 9, dtype=torch.int32, device="cuda:0") if with_status else None
    ctx.env_perturb(None if mask is None else torch.from_numpy(mask).cuda(), torch.from_numpy(recs).cuda(), status)
    ctx.synchronize()
    ep, es = ctx.env_get_state()
    return ep, es, status.cpu().numpy() if with_status else None


def test_rows_written_and_everything_else_left_alone(model):
    N = N_ROWS
    cfg = L.default_config(num_envs=N, batch_size=N)          # randomisers and noise on: the untouched columns hold draws
    ctx, torch = _ctx(model, cfg)
    ctx.env_reset_all(11, *_obs(torch, N))
    ctx.synchronize()
    ep0, es0 = ctx.env_get_state()
    assert (ep0[:, EP["JPBIAS"]:EP["LATENCY"]] != 0).all(1).any() and len(np.unique(ep0[:, EP["KP"]])) > N // 2
    rng = np.random.default_rng(4)
    recs = _records(rng, N)
    mask = rng.choice(np.array([0, 0, 1, 1, 2.5, -1], np.float32), N)
    mask[:4] = [1, 0, 1, 0]
    mask[4:13], recs[4:13, P["LATENCY"]] = 1, [-1, -0.5, -3, 0, 1, 2, 3, 4, 5]
    m = mask != 0
    assert set(recs[m, P["LATENCY"]]) >= {-1, -0.5, 0, 5} and 10 < m.sum() < N - 10
    ep1, es1, status = _perturb(ctx, torch, mask, recs)
    want = RR.perturbed_rows(model, recs, ep0, mask)
    assert np.array_equal(_bits(ep1), _bits(want)), np.argwhere(_bits(ep1) != _bits(want))[:8]
    assert np.array_equal(_bits(ep1[~m]), _bits(ep0[~m])), "an unmasked row was touched"
    assert np.array_equal(_bits(ep1[m][:, RR.KEPT]), _bits(ep0[m][:, RR.KEPT])), "JPBIAS / PGBIAS / PGLAG / the tail were touched"
    keep = m & (recs[:, P["LATENCY"]] < 0)
    assert np.array_equal(_bits(ep1[keep, EP["LATENCY"]]), _bits(ep0[keep, EP["LATENCY"]])) and np.array_equal(ep1[m & ~keep, EP["LATENCY"]], recs[m & ~keep, P["LATENCY"]])
    assert (_bits(ep1[m][:, RR.WRITTEN]) != _bits(ep0[m][:, RR.WRITTEN])).mean() > 0.5          # the call did something
    assert np.array_equal(_bits(es1), _bits(es0)), "the env state was touched"
    assert np.array_equal(status, np.where(m, 1, 0))
    # mask_d = NULL: every env, other records, over the rows the first call left; then without status_d
    recs2 = _records(rng, N)
    ep2, es2, status2 = _perturb(ctx, torch, None, recs2)
    want2 = RR.perturbed_rows(model, recs2, ep1)
    assert np.array_equal(_bits(ep2), _bits(want2)) and np.array_equal(_bits(es2), _bits(es0)) and (status2 == 1).all()
    assert np.array_equal(_bits(ep2[:, RR.KEPT]), _bits(ep0[:, RR.KEPT]))
    ep3, _, _ = _perturb(ctx, torch, mask, recs, with_status=False)
    assert np.array_equal(_bits(ep3), _bits(RR.perturbed_rows(model, recs, ep2, mask)))
    # the identity record: the row the reset path writes with the randomisers off, latency and sensor draws kept
    ep4, _, _ = _perturb(ctx, torch, None, np.tile(RR.identity_record(), (N, 1)))
    ctx.close()
    ctx, torch = _ctx(model, L.default_config(num_envs=N, batch_size=N, enable_randomizers=0))
    ctx.env_reset_all(11, *_obs(torch, N))
    ctx.synchronize()
    nominal, _ = ctx.env_get_state()
    ctx.close()
    assert np.array_equal(_bits(ep4[:, RR.WRITTEN]), _bits(nominal[:, RR.WRITTEN])) and np.array_equal(_bits(ep4[:, RR.KEPT]), _bits(ep0[:, RR.KEPT]))
    assert np.array_equal(_bits(ep4[:, EP["LATENCY"]]), _bits(ep3[:, EP["LATENCY"]]))


def test_refusals(model):
    from kbot_joystick_amd.host import binding as B
    N = 24
    ctx, torch = _ctx(model, L.default_config(num_envs=N, batch_size=N))
    ctx.env_reset_all(5, *_obs(torch, N))
    ctx.synchronize()
    ep0, es0 = ctx.env_get_state()
    recs = _records(np.random.default_rng(9), N)
    nan, inf = np.float32("nan"), np.float32("inf")
    bad = {1: (P["MASS_SCALE"], 0.0), 3: (P["MASS_SCALE"], -1.0), 5: (P["MU_SCALE"], 0.0), 7: (P["ARMATURE_SCALE"], -0.5), 9: (P["FRICLOSS_SCALE"], -0.1),
           11: (P["PAYLOAD"], -1.0), 12: (P["KP_SCALE"] + 19, 0.0), 13: (P["KD_SCALE"] + 4, -0.25), 15: (P["TAULIM_SCALE"] + 7, 0.0), 16: (P["ACTBIAS"] + 19, nan),
           17: (P["COM_SHIFT"] + 1, inf), 19: (P["LATENCY"], 2.5), 20: (P["LATENCY"], nan), 21: (P["LATENCY"], -inf), 23: (P["KD_SCALE"], inf)}
    for env, (slot, value) in bad.items():
        recs[env, slot] = value
    ep1, es1, status = _perturb(ctx, torch, None, recs)
    refused = np.zeros(N, bool)
    refused[list(bad)] = True
    assert np.array_equal(status, np.where(refused, -1, 1)) and np.array_equal(status, RR.status_ref(recs))
    assert np.array_equal(_bits(ep1[refused]), _bits(ep0[refused])), "a refused record changed its row"
    assert np.array_equal(_bits(ep1), _bits(RR.perturbed_rows(model, recs, ep0))) and (_bits(ep1[~refused]) != _bits(ep0[~refused])).any(1).all()      # the neighbours were written
    assert np.array_equal(_bits(es1), _bits(es0))
    # argument errors, before anything is launched
    pert = torch.from_numpy(np.tile(RR.identity_record(), (N + 1, 1))).cuda()
    status_d = torch.full((N,), 9, dtype=torch.int32, device="cuda:0")
    with pytest.raises(B.KbjError, match="kbj_env_perturb: null argument"):
        ctx.env_perturb(None, None, status_d)
    for off in (4, 8, 12):
        with pytest.raises(B.KbjError, match="kbj_env_perturb: pert_d must be 16-byte aligned"):
            ctx.env_perturb(None, pert.data_ptr() + off, status_d)
    assert B.load_library().kbj_env_perturb(None, None, pert.data_ptr(), status_d.data_ptr()) < 0      # a NULL ctx
    ctx.synchronize()
    ep2, _ = ctx.env_get_state()
    assert (status_d.cpu().numpy() == 9).all() and np.array_equal(_bits(ep2), _bits(ep1))
    ctx.env_perturb(None, pert, status_d)                                                               # the context is still usable
    ctx.synchronize()
    assert (status_d.cpu().numpy() == 1).all()
    ctx.close()


def test_step_kernel_under_perturbed_rows_matches_the_oracle(model):
    """The seven dynamics cases and nominal (tests/robustness_ref.py dynamics_cases: friction x 0.3, mass x 1.3, payload 8 kg, kp x 0.6,
    torque x 0.5, latency 5, armature x 2 with latency 0), 8 envs each, 20 teacher-forced steps of 64 envs. The records go in through
    kbj_env_perturb before step 0 and the device keeps stepping under the rows IT wrote (kbj_env_set_state gets the state alone); both
    oracles get perturbed_row's rows. That each case moves the oracle by far more than the tolerance is
    tests/test_robustness_host.py::test_every_dynamics_case_moves_the_oracle."""
    made = {}

    def make(cfg, seed, ep_reset, records):
        ctx, torch = _ctx(model, cfg)
        N = cfg.num_envs
        a, c, x = _obs(torch, N)
        ctx.env_reset_all(seed, a, c, x)
        ctx.synchronize()
        assert np.array_equal(_bits(ctx.env_get_state()[0]), _bits(ep_reset)), "the reset rows differ from the oracle's"
        rows, _, status = _perturb(ctx, torch, None, records)
        assert (status == 1).all()
        made["ctx"] = ctx

        def step(ep0, es0, act, aux_in):
            ctx.env_set_state(None, es0)
            aux_t = torch.from_numpy(aux_in.copy()).cuda()
            ctx.env_step(torch.from_numpy(act).cuda(), aux_t, a, c, x)
            ctx.synchronize()
            ep, es = ctx.env_get_state()
            return H.Step(ep, es, aux_t.cpu().numpy(), a.cpu().numpy(), c.cpu().numpy(), x.cpu().numpy())
        return rows, step

    errs, errs_o, left_out, got, want = RR.dynamics_run(model, make)
    final_ep = made["ctx"].env_get_state()[0]
    made["ctx"].close()
    print("hip vs oracle fp32:", RR.quantiles(errs))
    print("oracle fp32 vs fp64:", RR.quantiles(errs_o))
    assert np.array_equal(_bits(got), _bits(want)), "kbj_env_perturb's rows differ from perturbed_row's"
    assert np.array_equal(_bits(final_ep), _bits(want)), "the rows did not survive the steps"
    assert left_out == 0, f"{left_out} env-steps ended an episode: none does on the oracle in this setup"
    H.check_error_distribution(errs_o, label="perturbed: oracle fp32 vs fp64 ")
    H.check_error_distribution(errs, label="perturbed: hip vs oracle fp32 ")
