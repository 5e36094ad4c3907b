"""The step-response sweep end to end through HumanoidWalkingTask: 3 transitions x 2 repeats on freshly initialised parameters, every episode
cut after 9 steps so that envs reset inside the run, in front of the step and behind it. Checked: the command columns of the aux rows hold the
schedule on every row of every env; rec and stats are the restatement's on the returned signal, bit for bit; every entry's counts add up;
the table formats; a second sweep returns the same bytes. No claim about the outcomes: an untrained policy mostly falls or is VOID."""
import numpy as np
import pytest

from kbot_joystick_amd.spec import layout as L
from tests import step_response_ref as SR

pytestmark = pytest.mark.gpu
G_, R, S, O, X = L.SSIG, L.SREC, L.SSTAT, L.SOUT, L.AUX


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_step_sweep_end_to_end():
    from kbot_joystick_amd.host import step
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
    cfg = launch_config(num_envs=32, batch_size=32, hidden_size=64, num_passes=1, rollout_length_seconds=12 * 0.02, robot="kbot-headless", seed=5,
                        termination_params={"episode_length": {"max_length_sec": 9 * 0.02}})      # time-outs on rows 8, 17, 26 ..: none on the five rows in front of the step
    task = HumanoidWalkingTask(cfg)
    transitions = [((), (0.6,)), ((0.6,), ()), ((0.0, 0.0, 0.5), (0.0, 0.0, -0.5))]
    kw = dict(step_at=0.3, window=0.6, hold=0.1, smooth=0.1, repeats=2)
    entries, rec = task.step_sweep(transitions, **kw)
    row, win, hold, m = 15, 30, 5, 5
    T, N = row + win, 6
    aux, sig, sched = rec.aux.cpu().numpy(), rec.sig.cpu().numpy(), rec.sched.cpu().numpy()
    assert aux.shape == (T + 1, N, X["SIZE"]) and sig.shape == (T, N, G_["SIZE"]) and np.array_equal(sched, np.full(N, row, np.int32))
    done = aux[:T, :, X["DONE"]] != 0
    assert done[:row].any() and done[row:].any(), "no env was reset inside the run: the schedule's survival of a reset is not exercised"
    for e in range(N):
        c0, c1 = (np.zeros(L.NCMD, np.float32) for _ in range(2))
        c0[:len(transitions[e % 3][0])], c1[:len(transitions[e % 3][1])] = transitions[e % 3][0], transitions[e % 3][1]
        assert (aux[:row, e, X["CMD"]:X["CMD"] + L.NCMD] == c0).all() and (aux[row:, e, X["CMD"]:X["CMD"] + L.NCMD] == c1).all(), e
    assert np.array_equal(_bits(sig[..., G_["CMD"]:G_["CMD"] + 3]), _bits(aux[:T, :, X["CMD"]:X["CMD"] + 3])) and np.array_equal(_bits(sig[..., G_["DONE"]]), _bits(aux[:T, :, X["DONE"]]))
    bound = SR.signal_bound(aux, T)
    assert (np.abs(sig[..., :2].astype(np.float64) - SR.signal_ref(aux, T)[..., :2]) <= bound[..., None]).all()
    x = entries[0]
    crit = SR.Criteria(x["min_step"], x["band_abs"], x["band_frac"], x["rise_level"], m, hold, win)
    dt = task.config.ctrl_dt
    assert (x["step_at"], x["window"], x["hold"], x["smooth"], x["repeats"]) == (row * dt, win * dt, hold * dt, m * dt, 2) and x["rise_level"] == 0.9
    want_rec, want = SR.step_response_ref(sig, sched, crit, np.arange(N) % 3, 3)
    assert np.array_equal(_bits(rec.rec.cpu().numpy()), _bits(want_rec))
    assert np.array_equal(rec.stats.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert (want_rec[:, R["OUTCOME"]] != O["NONE"]).all()
    for i, e in enumerate(entries):
        cnt = want[i, S["COUNT"]:S["COUNT"] + O["COUNT"]]
        assert cnt.sum() == 2 and e["valid"] + e["void"] == 2 and e["void"] == cnt[O["VOID"]]
        assert e["from_command"][:3] == tuple(np.float32(v) for v in (list(transitions[i][0]) + [0, 0, 0])[:3])
        for name in ("fell", "settled", "unsettled", "censored"):
            f = e[name + "_frac"]
            assert (np.isnan(f) and e["valid"] == 0) or f == cnt[O[name.upper()]] / e["valid"]
    text = step.format_step_table(entries)
    print(text)
    assert len(text.splitlines()) == 5 and "(zero) -> xvel=+0.60" in text and "yawrate=+0.50 -> yawrate=-0.50" in text and "settings, not measured thresholds" in text
    entries2, rec2 = task.step_sweep(transitions, **kw)
    assert entries2 == entries or all(a == b or (a != a and b != b) for x2, x1 in zip(entries2, entries) for a, b in zip(x2.values(), x1.values()))
    for name in ("aux", "sig", "rec", "stats", "sched"):
        assert getattr(rec, name).cpu().numpy().tobytes() == getattr(rec2, name).cpu().numpy().tobytes(), name
    with pytest.raises(ValueError, match="at most 32 rows"):
        task.step_sweep(transitions, smooth=0.7)
    task.close()
