"""kbj_frequency_response on the GPU against tests/frequency_response_ref.py, driven through the C ABI on synthetic aux rows (no env step): N = 130
(two full wavefronts and a ragged one of 2), T = 333 (a multiple of no chunk; room for P = 256 behind its 64 lead rows), periods 4, 8, 12, 64
and 256, 1, 3 and INT32_MAX whole periods, 1, 3 and 256 groups.

sig_d: byte for byte what kbj_step_response writes for the same aux rows (it is the same stage). rec_d and stats_d: bit for bit against the
restatement run on the device's OWN sig_d (everything behind stage 1 is an exact function of it: whole numbers, fp32 extrema, float64 sums
of exact products in a fixed order); where the restatement's word is a NaN the device's is a NaN. The same bytes on a second call, with
stats_d NULL and with a rec_d that is only 8-byte aligned; the guard bands around the three outputs untouched."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import frequency_response_ref as FR

pytestmark = pytest.mark.gpu
G_, R, S, O = L.SSIG, L.FREC, L.FSTAT, L.FOUT
T, N = FR.T_SYN, FR.N_SYN
GUARD = 64            # words in front of and behind every output (16-byte alignment kept)


@pytest.fixture(scope="module")
def sctx():
    import torch
    from kbot_joystick_amd.host import binding as B
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=64, batch_size=64, hidden_size=64, rollout_len=8), 0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def prob():
    import torch
    p = FR.problem()
    return p, torch.from_numpy(p.aux).to("cuda:0"), torch.from_numpy(p.sched).to("cuda:0")


def _crit(min_amp=FR.MIN_AMP):
    from kbot_joystick_amd.host import binding as B
    return B.FrequencyCriteria((B.C.c_float * L.NSCH)(*min_amp))


class _Guarded:
    """A device buffer of `words` words between two guard bands filled with `fill`; `shift` words of the front band go to the body's
    address instead (an output that is 8-byte but not 16-byte aligned)."""
    def __init__(self, torch, words, dtype, fill, shift=0):
        self.all = torch.full((words + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
        self.lo, self.fill = GUARD + shift, fill
        self.body = self.all[self.lo:self.lo + words]

    def intact(self):
        a = self.all.cpu().numpy()
        return (a[:self.lo] == self.fill).all() and (a[self.lo + len(self.body):] == self.fill).all()


def _run(ctx, aux_d, sched_d, G, with_stats=True, fill=-7.0, group=True, rec_shift=0):
    import torch
    from kbot_joystick_amd.host import binding as B
    sig, rec = _Guarded(torch, T * N * G_["SIZE"], torch.float32, fill), _Guarded(torch, N * R["SIZE"], torch.float64, fill, rec_shift)
    stats = _Guarded(torch, G * S["SIZE"], torch.float64, fill) if with_stats else None
    group_d = torch.from_numpy(FR.groups(N, G)).to("cuda:0") if group else None
    ctx.frequency_response(B.Traj(T=T, N=N, aux_d=aux_d.data_ptr()), sched_d, _crit(), sig.body, rec.body, group_d, G, stats.body if with_stats else None)
    ctx.synchronize()
    assert sig.intact() and rec.intact() and (stats is None or stats.intact()), "a guard band was written"
    return (sig.body.cpu().numpy().reshape(T, N, G_["SIZE"]), rec.body.cpu().numpy().reshape(N, R["SIZE"]),
            stats.body.cpu().numpy().reshape(G, S["SIZE"]) if with_stats else None)


def _where(got, want):
    bad = ~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want)))
    return np.argwhere(bad)[:8], got[bad][:8], want[bad][:8]


def test_frequency_response_matches_the_restatement(sctx, prob):
    import torch
    from kbot_joystick_amd.host import binding as B
    from tests import step_response_ref as SR
    p, aux_d, sched_d = prob
    sig, rec, stats = _run(sctx, aux_d, sched_d, 3)
    # stage 1 is kbj_step_response's: the same bytes for the same aux rows
    f3 = B.C.c_float * L.NSCH
    step_sig, step_rec = torch.full((T, N, G_["SIZE"]), -7.0, device="cuda:0"), torch.full((N, L.SREC["SIZE"]), -7.0, device="cuda:0")
    sctx.step_response(B.Traj(T=T, N=N, aux_d=aux_d.data_ptr()), torch.full((N,), 20, dtype=torch.int32, device="cuda:0"),
                       B.StepCriteria(f3(*SR.BASE["min_step"]), f3(*SR.BASE["band_abs"]), 0.25, 0.75, 3, 4, 30), step_sig, step_rec)
    sctx.synchronize()
    assert step_sig.cpu().numpy().tobytes() == sig.tobytes()
    # stage 2 on the device's own signal
    want_rec, _ = FR.scan_ref(sig, p.sched, FR.MIN_AMP)
    assert FR.same_words(rec, want_rec), _where(rec, want_rec)
    oc = rec[:, R["OUTCOME"]]
    assert all((oc == O[k]).sum() >= 5 for k in ("NONE", "VOID", "FELL", "MEASURED", "FLAT", "CENSORED")), np.bincount(oc.astype(int))
    assert np.isnan(want_rec).any() and np.isnan(rec[oc == O["MEASURED"]]).any()                   # the NaN samples reached the sums
    for G in (1, 3, 256):
        sig_g, rec_g, stats_g = (sig, rec, stats) if G == 3 else _run(sctx, aux_d, sched_d, G)
        assert sig_g.tobytes() == sig.tobytes() and rec_g.tobytes() == rec.tobytes()
        want = FR.group_stats_ref(want_rec, FR.groups(N, G), G)
        assert FR.same_words(stats_g, want), (G,) + _where(stats_g, want)
    sig2, rec2, stats2 = _run(sctx, aux_d, sched_d, 3, fill=3.0)           # a second call, over other bytes
    assert sig2.tobytes() == sig.tobytes() and rec2.tobytes() == rec.tobytes() and stats2.tobytes() == stats.tobytes()
    sig3, rec3, _ = _run(sctx, aux_d, sched_d, 3, with_stats=False)
    assert sig3.tobytes() == sig.tobytes() and rec3.tobytes() == rec.tobytes()
    _, _, stats4 = _run(sctx, aux_d, sched_d, 1, group=False)              # group_d = NULL: every env in group 0
    want4 = FR.group_stats_ref(want_rec, None, 1)
    assert FR.same_words(stats4, want4), _where(stats4, want4)
    _, rec5, stats5 = _run(sctx, aux_d, sched_d, 3, rec_shift=1)           # rec_d on an odd multiple of 8 bytes: kbj.h asks no more of it
    assert rec5.tobytes() == rec.tobytes() and stats5.tobytes() == stats.tobytes()


def test_frequency_response_reports_every_argument_error(sctx, prob):
    import torch
    from kbot_joystick_amd.host import binding as B
    p, aux_d, sched_d = prob
    sig = torch.full((T * N * G_["SIZE"] + 4,), -7.0, device="cuda:0")
    rec = torch.full((N * R["SIZE"] + 2,), -7.0, dtype=torch.float64, device="cuda:0")
    stats = torch.full((2 * S["SIZE"] + 2,), -7.0, dtype=torch.float64, device="cuda:0")
    sched_pad = torch.cat([torch.zeros(1, 4, dtype=torch.int32, device="cuda:0"), sched_d])        # + 4 bytes: not 16-byte aligned
    traj = B.Traj(T=T, N=N, aux_d=aux_d.data_ptr())
    nan = float("nan")
    good = dict(traj=traj, sched=sched_d, criteria=_crit(), sig=sig, rec=rec, group=None, G=2, stats=stats)
    bad = [(dict(traj=None), "null argument"), (dict(sched=None), "null argument"), (dict(criteria=None), "null argument"), (dict(sig=None), "null argument"),
           (dict(rec=None), "null argument"), (dict(traj=B.Traj(T=T, N=N)), "needs aux_d"), (dict(traj=B.Traj(T=0, N=N, aux_d=aux_d.data_ptr())), "positive T, N"),
           (dict(traj=B.Traj(T=T, N=0, aux_d=aux_d.data_ptr())), "positive T, N"), (dict(traj=B.Traj(T=T, N=N, aux_d=aux_d.data_ptr() + 4)), "16-byte aligned"),
           (dict(sig=sig.data_ptr() + 4), "16-byte aligned"), (dict(sched=sched_pad.data_ptr() + 4), "16-byte aligned"), (dict(sched=sched_pad.data_ptr() + 8), "16-byte aligned"),
           (dict(rec=rec.data_ptr() + 4), "8-byte aligned"), (dict(stats=stats.data_ptr() + 4), "8-byte aligned"),
           (dict(criteria=_crit((-0.1, 0.1, 0.1))), "min_amp is negative or NaN"), (dict(criteria=_crit((0.1, nan, 0.1))), "min_amp is negative or NaN"),
           (dict(criteria=_crit((0.1, 0.1, -1.0))), "min_amp is negative or NaN"), (dict(G=0), r"G must be in \[1, 256\]"), (dict(G=257), r"G must be in \[1, 256\]")]
    for change, msg in bad:
        with pytest.raises(B.KbjError, match=msg):
            sctx.frequency_response(**dict(good, **change))
    lib = B.load_library()
    assert lib.kbj_frequency_response(None, B.C.byref(traj), sched_d.data_ptr(), B.C.byref(_crit()), sig.data_ptr(), rec.data_ptr(), None, 2, stats.data_ptr()) < 0     # a NULL ctx
    sctx.synchronize()
    assert (sig.cpu().numpy() == -7).all() and (rec.cpu().numpy() == -7).all() and (stats.cpu().numpy() == -7).all()         # nothing was launched
    sctx.frequency_response(**dict(good, G=300, stats=None))                             # without stats_d, G is not read
    sctx.frequency_response(**good)                                                      # the context is still usable
    sctx.synchronize()
    got = rec.cpu().numpy()[:N * R["SIZE"]].reshape(N, R["SIZE"])
    want, _ = FR.scan_ref(sig.cpu().numpy()[:T * N * G_["SIZE"]].reshape(T, N, G_["SIZE"]), p.sched, FR.MIN_AMP)
    assert FR.same_words(got, want) and (stats.cpu().numpy()[:2 * S["SIZE"]] != -7).all()
    assert (sig.cpu().numpy()[-4:] == -7).all() and (rec.cpu().numpy()[-2:] == -7).all() and (stats.cpu().numpy()[-2:] == -7).all()
