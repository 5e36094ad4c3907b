"""kbj_step_response on the GPU against tests/step_response_ref.py, driven through the C ABI on synthetic aux rows (no env step): N = 130 (two
full wavefronts and a ragged one of 2), T = 75 (a multiple of no chunk), smoothing over 1, 3 and 32 rows, hold 1 and 4, 1, 3 and 256 groups,
a window of 30 rows and of INT32_MAX.

Bounds. VX and VY of sig_d: within signal_bound of the float64 signal - (|vx| + |vy|) 2^-24 (8 + 6 M / h), derived there from the operation
count of stage 1, not from what the kernel gives; where the float64 signal is NaN the device's is too. WZ, DONE, CMD and the spare word:
bit for bit. rec_d and stats_d: bit for bit against the restatement run on the device's OWN sig_d (everything behind stage 1 is an exact
function of it). The same bytes on a second call and with stats_d NULL; the guard bands around the three outputs untouched."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import step_response_ref as SR

pytestmark = pytest.mark.gpu
G_, R, S, O, X = L.SSIG, L.SREC, L.SSTAT, L.SOUT, L.AUX
T, N = SR.T_SYN, SR.N_SYN
GUARD = 64            # words in front of and behind every output (16-byte alignment kept)
COMBOS = [(m, hold) for m in (1, 3, 32) for hold in (1, 4)]


@pytest.fixture(scope="module")
def sctx():
    import torch
    from kbot_joystick_amd.host import binding as B
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=64, batch_size=64, hidden_size=64, rollout_len=8), 0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _crit(c: SR.Criteria):
    from kbot_joystick_amd.host import binding as B
    f3 = B.C.c_float * L.NSCH
    return B.StepCriteria(f3(*c.min_step), f3(*c.band_abs), c.band_frac, c.rise_level, c.smooth, c.hold, c.window)


class _Guarded:
    """A device buffer of `words` words between two guard bands filled with `fill`."""
    def __init__(self, torch, words, dtype, fill):
        self.all = torch.full((words + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
        self.body, self.fill = self.all[GUARD:GUARD + words], fill

    def intact(self):
        a = self.all.cpu().numpy()
        return (a[:GUARD] == self.fill).all() and (a[-GUARD:] == self.fill).all()


def _run(ctx, aux_d, sched_d, crit: SR.Criteria, G, with_stats=True, fill=-7.0, group=True):
    import torch
    from kbot_joystick_amd.host import binding as B
    sig, rec = _Guarded(torch, T * N * G_["SIZE"], torch.float32, fill), _Guarded(torch, N * R["SIZE"], torch.float32, fill)
    stats = _Guarded(torch, G * S["SIZE"], torch.float64, fill) if with_stats else None
    group_d = torch.from_numpy(SR.groups(N, G)).to("cuda:0") if group else None
    ctx.step_response(B.Traj(T=T, N=N, aux_d=aux_d.data_ptr()), sched_d, _crit(crit), sig.body, rec.body, group_d, G, stats.body if with_stats else None)
    ctx.synchronize()
    assert sig.intact() and rec.intact() and (stats is None or stats.intact()), "a guard band was written"
    return (sig.body.cpu().numpy().reshape(T, N, G_["SIZE"]), rec.body.cpu().numpy().reshape(N, R["SIZE"]),
            stats.body.cpu().numpy().reshape(G, S["SIZE"]) if with_stats else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_signal(sig, aux):
    want, bound = SR.signal_ref(aux, T), SR.signal_bound(aux, T)
    a32 = aux[:T]
    assert np.array_equal(_bits(sig[..., G_["WZ"]]), _bits(a32[..., X["QVEL"] + 5])) and np.array_equal(_bits(sig[..., G_["DONE"]]), _bits(a32[..., X["DONE"]]))
    assert np.array_equal(_bits(sig[..., G_["CMD"]:G_["CMD"] + 3]), _bits(a32[..., X["CMD"]:X["CMD"] + 3])) and (_bits(sig[..., G_["SPARE"]]) == 0).all()
    worst = 0.0
    for k in (G_["VX"], G_["VY"]):
        nan = np.isnan(want[..., k])
        assert np.array_equal(np.isnan(sig[..., k]), nan)
        err = np.abs(sig[..., k].astype(np.float64) - want[..., k])
        ok = nan | (err <= bound)
        assert ok.all(), (k, np.argwhere(~ok)[:5], err[~ok][:5], bound[~ok][:5])
        worst = max(worst, float(np.max(np.where(nan | (bound == 0), 0.0, err / np.where(bound > 0, bound, 1.0)))))
    exact = bound == 0                                  # the degenerate heading: (c, s) = (1, 0), the velocity passes through
    assert exact.any() and np.array_equal(_bits(sig[..., 0][exact]), _bits(a32[..., X["QVEL"]][exact])) and np.array_equal(_bits(sig[..., 1][exact]), _bits(a32[..., X["QVEL"] + 1][exact]))
    return worst


@pytest.mark.parametrize("m,hold", COMBOS)
def test_step_response_matches_the_restatement(sctx, m, hold):
    import torch
    prob = SR.problem(hold)
    aux_d, sched_d = torch.from_numpy(prob.aux).to("cuda:0"), torch.from_numpy(prob.sched).to("cuda:0")
    crit = SR.criteria(m, hold)
    sig, rec, stats = _run(sctx, aux_d, sched_d, crit, 3)
    worst = _check_signal(sig, prob.aux)
    print(f"m={m} hold={hold}: largest signal error / bound {worst:.3f}")
    want_rec, _ = SR.scan_ref(sig, prob.sched, crit)                        # on the device's own signal
    assert np.array_equal(_bits(rec), _bits(want_rec)), (np.argwhere(_bits(rec) != _bits(want_rec))[:8], rec[_bits(rec) != _bits(want_rec)][:8], want_rec[_bits(rec) != _bits(want_rec)][:8])
    oc = rec[:, R["OUTCOME"]]
    assert all((oc == O[k]).sum() >= 5 for k in ("NONE", "VOID", "FELL", "SETTLED", "UNSETTLED", "CENSORED")), np.bincount(oc.astype(int))
    for G in (1, 3, 256):
        sig_g, rec_g, stats_g = (sig, rec, stats) if G == 3 else _run(sctx, aux_d, sched_d, crit, G)
        assert sig_g.tobytes() == sig.tobytes() and rec_g.tobytes() == rec.tobytes()
        want = SR.group_stats_ref(want_rec, SR.groups(N, G), G)
        assert np.array_equal(stats_g.view(np.uint64), want.view(np.uint64)), (G, np.argwhere(stats_g.view(np.uint64) != want.view(np.uint64))[:8])
    sig2, rec2, stats2 = _run(sctx, aux_d, sched_d, crit, 3, fill=3.0)      # a second call, over other bytes
    assert sig2.tobytes() == sig.tobytes() and rec2.tobytes() == rec.tobytes() and stats2.tobytes() == stats.tobytes()
    sig3, rec3, _ = _run(sctx, aux_d, sched_d, crit, 3, with_stats=False)
    assert sig3.tobytes() == sig.tobytes() and rec3.tobytes() == rec.tobytes()
    _, _, stats4 = _run(sctx, aux_d, sched_d, crit, 1, group=False)         # group_d = NULL: every env in group 0
    assert np.array_equal(stats4.view(np.uint64), SR.group_stats_ref(want_rec, None, 1).view(np.uint64))
    # a window of INT32_MAX rows: s + window is taken in 64 bits; nothing is UNSETTLED any more, the trajectory cuts every open window
    wide = SR.criteria(m, hold, SR.INT32_MAX)
    _, rec5, stats5 = _run(sctx, aux_d, sched_d, wide, 3)
    want5, _ = SR.scan_ref(sig, prob.sched, wide)
    assert np.array_equal(_bits(rec5), _bits(want5)) and (rec5[:, R["OUTCOME"]] != O["UNSETTLED"]).all() and not np.array_equal(_bits(rec5), _bits(rec))
    assert np.array_equal(stats5.view(np.uint64), SR.group_stats_ref(want5, SR.groups(N, 3), 3).view(np.uint64))


def test_step_response_reports_every_argument_error(sctx):
    import torch
    from kbot_joystick_amd.host import binding as B
    prob = SR.problem(4)
    aux_d, sched_d = torch.from_numpy(prob.aux).to("cuda:0"), torch.from_numpy(prob.sched).to("cuda:0")
    sig, rec = torch.full((T * N * G_["SIZE"] + 4,), -7.0, device="cuda:0"), torch.full((N * R["SIZE"] + 4,), -7.0, device="cuda:0")
    stats = torch.full((2, S["SIZE"]), -7.0, dtype=torch.float64, device="cuda:0")
    traj = B.Traj(T=T, N=N, aux_d=aux_d.data_ptr())
    base = SR.criteria(3, 4)
    nan = float("nan")
    good = dict(traj=traj, sched=sched_d, criteria=_crit(base), sig=sig, rec=rec, group=None, G=2, stats=stats)
    bad = [(dict(traj=None), "null argument"), (dict(sched=None), "null argument"), (dict(criteria=None), "null argument"), (dict(sig=None), "null argument"),
           (dict(rec=None), "null argument"), (dict(traj=B.Traj(T=T, N=N)), "needs aux_d"), (dict(traj=B.Traj(T=0, N=N, aux_d=aux_d.data_ptr())), "positive T, N"),
           (dict(traj=B.Traj(T=T, N=0, aux_d=aux_d.data_ptr())), "positive T, N"), (dict(traj=B.Traj(T=T, N=N, aux_d=aux_d.data_ptr() + 4)), "16-byte aligned"),
           (dict(sig=sig.data_ptr() + 4), "16-byte aligned"), (dict(rec=rec.data_ptr() + 4), "16-byte aligned"),
           (dict(criteria=_crit(base._replace(smooth=0))), r"smooth_steps must be in \[1, 32\]"), (dict(criteria=_crit(base._replace(smooth=33))), r"smooth_steps must be in \[1, 32\]"),
           (dict(criteria=_crit(base._replace(hold=0))), "hold_steps"), (dict(criteria=_crit(base._replace(window=0))), "window_steps"),
           (dict(criteria=_crit(base._replace(rise_level=0.0))), r"rise_level must be in \(0, 1\]"), (dict(criteria=_crit(base._replace(rise_level=1.5))), "rise_level"),
           (dict(criteria=_crit(base._replace(rise_level=nan))), "rise_level"), (dict(criteria=_crit(base._replace(band_frac=-0.5))), "band_frac"),
           (dict(criteria=_crit(base._replace(band_frac=nan))), "band_frac"), (dict(criteria=_crit(base._replace(band_abs=(0.1, -0.1, 0.1)))), "band_abs"),
           (dict(criteria=_crit(base._replace(band_abs=(0.1, 0.1, nan)))), "band_abs"), (dict(criteria=_crit(base._replace(min_step=(-1.0, 0.1, 0.1)))), "min_step"),
           (dict(criteria=_crit(base._replace(min_step=(0.1, nan, 0.1)))), "min_step"), (dict(G=0), r"G must be in \[1, 256\]"), (dict(G=257), r"G must be in \[1, 256\]")]
    for change, msg in bad:
        with pytest.raises(B.KbjError, match=msg):
            sctx.step_response(**dict(good, **change))
    lib = B.load_library()
    assert lib.kbj_step_response(None, B.C.byref(traj), sched_d.data_ptr(), B.C.byref(_crit(base)), sig.data_ptr(), rec.data_ptr(), None, 2, stats.data_ptr()) < 0     # a NULL ctx
    sctx.synchronize()
    assert (sig.cpu().numpy() == -7).all() and (rec.cpu().numpy() == -7).all() and (stats.cpu().numpy() == -7).all()         # nothing was launched
    sctx.step_response(**dict(good, G=300, stats=None))                                  # without stats_d, G is not read
    sctx.step_response(**good)                                                           # the context is still usable
    sctx.synchronize()
    got = rec.cpu().numpy()[:N * R["SIZE"]].reshape(N, R["SIZE"])
    want, _ = SR.scan_ref(sig.cpu().numpy()[:T * N * G_["SIZE"]].reshape(T, N, G_["SIZE"]), prob.sched, base)
    assert np.array_equal(_bits(got), _bits(want)) and (stats.cpu().numpy() != -7).all()
    assert (sig.cpu().numpy()[-4:] == -7).all() and (rec.cpu().numpy()[-4:] == -7).all()
