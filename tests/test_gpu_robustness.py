"""kbj_robustness on the GPU against tests/robustness_ref.py, driven through the C ABI on synthetic err / aux rows (no env step): (T, N) =
(1, 1), (7, 5), (33, 70) and (130, 129) - one row, less than a chunk, a ragged chunk count with a ragged second wavefront, and three
wavefronts with one env in the last - with 1, 5 and 64 groups. The inputs hold groups outside [0, G), envs without a settled row, NaN and
negative errors, SETTLED flags other than 1 and every kind of DONE value.

rec_d and stats_d: bit for bit the sequential float64 sums (where the restatement's word is a NaN the device's is a NaN); the same bytes on a
second call and with stats_d NULL; the guard bands around both outputs untouched."""
import functools

import numpy as np
import pytest

from kbot_joystick_amd.spec import compiler, layout as L
from tests import robustness_ref as RR

pytestmark = pytest.mark.gpu
R, S, TE, X = L.RREC, L.RSTAT, L.TERR, L.AUX
SHAPES = [(1, 1), (7, 5), (33, 70), (130, 129)]
GUARD = 64            # words in front of and behind every output (16-byte alignment kept)


@pytest.fixture(scope="module")
def sctx():
    import torch
    from kbot_joystick_amd.host import binding as B
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = B.Context(compiler.load_model("kbot-headless"), L.default_config(num_envs=64, batch_size=64, hidden_size=64, rollout_len=8), 0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _problem(T, N):
    """The inputs of a shape and stage 1 of the restatement, computed once and shared by the group counts."""
    aux, err = RR.synthetic(T, N)
    return aux, err, RR.scan_ref(aux[:T, :, X["DONE"]], err)


class _Guarded:
    def __init__(self, torch, words, fill):
        self.all = torch.full((words + 2 * GUARD,), fill, dtype=torch.float64, device="cuda:0")
        self.fill, self.body = fill, self.all[GUARD:GUARD + words]

    def intact(self):
        a = self.all.cpu().numpy()
        return (a[:GUARD] == self.fill).all() and (a[GUARD + len(self.body):] == self.fill).all()


def _run(ctx, T, N, G, with_stats=True, fill=-7.0, group=True):
    import torch
    from kbot_joystick_amd.host import binding as B
    aux, err, _ = _problem(T, N)
    aux_d, err_d = torch.from_numpy(aux).cuda(), torch.from_numpy(err).cuda()
    rec = _Guarded(torch, N * R["SIZE"], fill)
    stats = _Guarded(torch, G * S["SIZE"], fill) if with_stats else None
    group_d = torch.from_numpy(RR.groups(N, G)).cuda() if group else None
    ctx.robustness(B.Traj(T=T, N=N, aux_d=aux_d.data_ptr()), err_d, rec.body, group_d, G, stats.body if with_stats else None)
    ctx.synchronize()
    assert rec.intact() and (stats is None or stats.intact()), "a guard band was written"
    return rec.body.cpu().numpy().reshape(N, R["SIZE"]), stats.body.cpu().numpy().reshape(G, S["SIZE"]) if with_stats else None


def _where(got, want):
    bad = ~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want)))
    return np.argwhere(bad)[:8], got[bad][:8], want[bad][:8]


@pytest.mark.parametrize("G", [1, 5, 64])
@pytest.mark.parametrize("T,N", SHAPES)
def test_robustness_matches_the_restatement(sctx, T, N, G):
    aux, err, want_rec = _problem(T, N)
    rec, stats = _run(sctx, T, N, G)
    assert RR.same_words(rec, want_rec), _where(rec, want_rec)
    want = RR.group_ref(want_rec, RR.groups(N, G), G)
    assert RR.same_words(stats, want), _where(stats, want)
    rec2, stats2 = _run(sctx, T, N, G, fill=3.0)                    # a second call, over other bytes
    assert rec2.tobytes() == rec.tobytes() and stats2.tobytes() == stats.tobytes()
    rec3, _ = _run(sctx, T, N, G, with_stats=False)
    assert rec3.tobytes() == rec.tobytes()
    _, stats4 = _run(sctx, T, N, G, group=False)                    # group_d = NULL: every env in group 0
    want4 = RR.group_ref(want_rec, None, G)
    assert RR.same_words(stats4, want4) and stats4[0, S["ENVS"]] == N and not stats4[1:, S["ENVS"]].any()


def test_the_inputs_cover_what_they_claim():
    T, N = SHAPES[-1]
    aux, err, rec = _problem(T, N)
    done = aux[:T, :, X["DONE"]]
    assert (done < 0).any() and (done > 0).any() and (done == 0).any() and ((done != np.floor(done)) & (done < 0)).any() and (done > 1).any()
    assert np.isnan(err[..., :L.NTERR]).any() and (err[..., :L.NTERR] < 0).any() and (err[..., TE["SETTLED"]] == 2).any()
    assert (rec[::4, R["SETTLED"]] == 0).all() and (rec[::4, R["ERR_MAX"]:R["ERR_MAX"] + 5] == -1).all() and np.isnan(rec[:, R["ERR_SUM"]]).any()
    assert np.isfinite(rec[2]).all() and rec[2, R["SETTLED"]] == T and (rec[:, R["FIRST_FALL"]] == -1).any() and (rec[:, R["FIRST_FALL"]] > 0).any()
    for G in (1, 5, 64):
        g = RR.groups(N, G)
        assert (g < 0).any() and (g >= G).any() and ((g >= 0) & (g < G)).any()
        stats = RR.group_ref(rec, g, G)
        assert stats[:, S["ENVS"]].sum() == ((g >= 0) & (g < G)).sum()
    assert (RR.group_ref(rec, RR.groups(N, 64), 64)[:, S["ENVS"]] == 0).any()          # a group without envs: its minimum and maxima stay -1


def test_robustness_reports_every_argument_error(sctx):
    import torch
    from kbot_joystick_amd.host import binding as B
    T, N = SHAPES[2]
    aux, err, want_rec = _problem(T, N)
    aux_d, err_d = torch.from_numpy(aux).cuda(), torch.cat([torch.from_numpy(err).reshape(-1), torch.zeros(4)]).cuda()
    rec = torch.full((N * R["SIZE"] + 2,), -7.0, dtype=torch.float64, device="cuda:0")
    stats = torch.full((2 * S["SIZE"] + 2,), -7.0, dtype=torch.float64, device="cuda:0")
    traj = B.Traj(T=T, N=N, aux_d=aux_d.data_ptr())
    good = dict(traj=traj, err=err_d, rec=rec, group=None, G=2, stats=stats)
    bad = [(dict(traj=None), "kbj_robustness: null argument"), (dict(err=None), "null argument"), (dict(rec=None), "null argument"),
           (dict(traj=B.Traj(T=T, N=N)), "needs aux_d"), (dict(traj=B.Traj(T=0, N=N, aux_d=aux_d.data_ptr())), "positive T, N"),
           (dict(traj=B.Traj(T=T, N=0, aux_d=aux_d.data_ptr())), "positive T, N"), (dict(err=err_d.data_ptr() + 4), "err_d and rec_d must be 16-byte aligned"),
           (dict(err=err_d.data_ptr() + 8), "16-byte aligned"), (dict(rec=rec.data_ptr() + 8), "16-byte aligned"), (dict(G=0), r"G must be in \[1, 256\]"),
           (dict(G=257), r"G must be in \[1, 256\]"), (dict(G=-3), r"G must be in \[1, 256\]")]
    for change, msg in bad:
        with pytest.raises(B.KbjError, match=msg):
            sctx.robustness(**dict(good, **change))
    assert B.load_library().kbj_robustness(None, B.C.byref(traj), err_d.data_ptr(), rec.data_ptr(), None, 2, stats.data_ptr()) < 0     # a NULL ctx
    sctx.synchronize()
    assert (rec.cpu().numpy() == -7).all() and (stats.cpu().numpy() == -7).all()         # nothing was launched
    sctx.robustness(**dict(good, G=300, stats=None))                                     # without stats_d, G is not read
    sctx.robustness(**good)                                                              # the context is still usable
    sctx.synchronize()
    got = rec.cpu().numpy()[:N * R["SIZE"]].reshape(N, R["SIZE"])
    assert RR.same_words(got, want_rec) and RR.same_words(stats.cpu().numpy()[:2 * S["SIZE"]].reshape(2, S["SIZE"]), RR.group_ref(want_rec, None, 2))
    assert (rec.cpu().numpy()[-2:] == -7).all() and (stats.cpu().numpy()[-2:] == -7).all()
