"""The frequency-response sweep end to end through HumanoidWalkingTask: 2 operating points x 2 periods (8 and 24 rows) x 2 repeats on freshly
initialised parameters, every episode cut after 50 steps so that envs reset inside the run, the sinusoid from row 3, T = 123 rows. Checked:
the driven command word of the aux rows - and the CMD words of the signal - hold SineCommand's value bit for bit on every row of every env,
the other words the base command; rec and stats are the restatement's on the returned signal; every entry is the host formulas on the
returned statistics; the table formats; the task's own context and a later scalars() call are unaffected. No claim about the figures: an
untrained policy mostly falls."""
import math

import numpy as np
import pytest

from kbot_joystick_amd.spec import constants, layout as L
from tests import frequency_response_ref as FR

pytestmark = pytest.mark.gpu
G_, R, S, O, X = L.SSIG, L.FREC, L.FSTAT, L.FOUT, L.AUX


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_frequency_sweep_end_to_end():
    from kbot_joystick_amd.host import frequency as F
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
    cfg = launch_config(num_envs=32, batch_size=32, hidden_size=64, num_passes=1, rollout_length_seconds=12 * 0.02, robot="kbot-headless", seed=5,
                        termination_params={"episode_length": {"max_length_sec": 50 * 0.02}})
    task = HumanoidWalkingTask(cfg)
    task.train_iteration()
    before = task.scalars()
    params = task.params.clone()
    points = [((), 0, 0.4), ((0.3, 0.0, 0.1), 2, 0.5)]
    periods = [8, 24]
    kw = dict(cycles=4, min_window=0.5, start_at=0.06, settle=0.06, min_amp=(0.05, 0.05, 0.1), repeats=2)
    entries, rec = task.frequency_sweep(points, periods, **kw)
    dt = task.config.ctrl_dt
    start, ncases, N = 3, 4, 8
    cases = [(0, 8, 11, 4), (0, 24, 27, 4), (1, 8, 11, 4), (1, 24, 27, 4)]          # point, P, s = 3 + ceil(3 / P) P, K = max(4, ceil(25 / P))
    T = 27 + 4 * 24
    aux, sig, sched = rec.aux.cpu().numpy(), rec.sig.cpu().numpy(), rec.sched.cpu().numpy()
    assert aux.shape == (T + 1, N, X["SIZE"]) and sig.shape == (T, N, G_["SIZE"]) and T < 150
    assert np.array_equal(sched, np.array([[s, P, points[i][1], K] for i, P, s, K in cases] * 2, np.int32))
    done = aux[:T, :, X["DONE"]] != 0
    assert done[start:].any(), "no env was reset inside the run: the schedule's survival of a reset is not exercised"
    for e in range(N):
        i, P, s, K = cases[e % ncases]
        base = np.zeros(L.NCMD, np.float32)
        base[:len(points[i][0])] = points[i][0]
        ch, amp = points[i][1], points[i][2]
        table = F.sine_table([base[ch]], [amp], [P])[0]
        want = np.tile(base, (T + 1, 1))
        want[:, ch] = table[np.maximum(np.arange(T + 1) - start, 0) % P]
        assert np.array_equal(aux[:, e, X["CMD"]:X["CMD"] + L.NCMD].view(np.uint32), want.view(np.uint32)), e
        assert np.array_equal(sig[:, e, G_["CMD"]:G_["CMD"] + 3].view(np.uint32), want[:T, :3].view(np.uint32)), e
    assert np.array_equal(sig[..., G_["DONE"]].view(np.uint32), aux[:T, :, X["DONE"]].view(np.uint32))
    want_rec, want = FR.frequency_response_ref(sig, sched, kw["min_amp"], np.arange(N) % ncases, ncases)
    got_rec, got = rec.rec.cpu().numpy(), rec.stats.cpu().numpy()
    assert got_rec.dtype == np.float64 and FR.same_words(got_rec, want_rec) and FR.same_words(got, want)
    oc = want_rec[:, R["OUTCOME"]]
    assert (oc >= O["VOID"]).all() and (want_rec[oc >= O["FELL"], R["PERIOD"]] == sched[oc >= O["FELL"], 1]).all()
    print("outcomes:", {name: int((oc == k).sum()) for k, name in enumerate(constants.FREQUENCY_OUTCOME_NAMES)})
    for c, e in enumerate(entries):
        i, P, s, K = cases[c]
        assert (e["point"], e["period_rows"], e["first_row"], e["periods"], e["channel"], e["amplitude"]) == (i, P, s, K, constants.STEP_CHANNEL_NAMES[points[i][1]], points[i][2])
        assert (e["start_at"], e["settle"], e["cycles"], e["repeats"], e["min_amp"]) == (3 * dt, 3 * dt, 4, 2, kw["min_amp"])
        cnt = want[c, S["COUNT"]:S["COUNT"] + O["COUNT"]]
        assert cnt.sum() == 2 and e["valid"] + e["void"] == 2 and e["void"] == cnt[O["VOID"]]
        for key, v in F.case_summary(got[c], points[i][1], P, dt).items():             # the host formulas on the returned statistics
            assert _same(e[key], v), (c, key, e[key], v)
        if cnt[O["MEASURED"]]:
            gain, lag, coh = FR.response_ref(want[c, S["ROWS"]], want[c, S["SUMS"]:S["SUMS"] + L.FREC_NSUMS], points[i][1])
            for a, b in ((e["gain"], gain), (math.radians(e["lag_deg"]), lag), (e["coherence"], coh)):
                assert _same(a, b) or abs(a - b) <= 1e-9 * max(1.0, abs(b)), (c, a, b)
        mine = [x for x in entries if x["point"] == i]
        bw, below = F.bandwidth_hz([x["frequency_hz"] for x in mine], [x["gain_db"] for x in mine])
        assert _same(e["bandwidth_hz"], bw) and e["bandwidth_below_range"] == below
    text = F.format_frequency_table(entries)
    print(text)
    lines = text.splitlines()
    assert len(lines) == 1 + 1 + 4 + 2 and "settings, not measured thresholds" in lines[0] and "(zero) forward +-0.40" in text and "yaw +-0.50" in text and "nan" not in text
    # the task's own context is untouched: the same scalars, the same parameters, and it trains on
    after = task.scalars()
    assert set(after) == set(before) and all(_same(after[k], before[k]) for k in before) and (task.params == params).all()
    task.train_iteration()
    assert np.isfinite(task.scalars()["train/loss"])
    task.close()
