"""The robustness sweep end to end through HumanoidWalkingTask: 3 perturbations (nominal, friction x 0.25, left-leg torque x 0.4) x 2 commands
(stand, forward) x 2 repeats on freshly initialised parameters, every episode cut after 25 steps so that every env restarts inside the 50
rows whatever the policy does. Checked: every env restarted; the model rows read back after the last step are perturbed_row of each env's
record (so the records were written AGAIN behind the in-step resets, which redraw the rows); rec and stats are the restatement's on the
record's own aux / err / group; every entry follows from its RSTAT vector; the table prints one line per case; a second call returns the
same bytes. No claim about the figures: an untrained policy mostly falls."""
import math

import numpy as np
import pytest

from kbot_joystick_amd.spec import constants, layout as L
from tests import robustness_ref as RR

pytestmark = pytest.mark.gpu
EP, P, R, S, X = L.EP, L.PERT, L.RREC, L.RSTAT, L.AUX


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_robustness_sweep_end_to_end():
    from kbot_joystick_amd.host import robustness as RB
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
    cfg = launch_config(num_envs=32, batch_size=32, hidden_size=64, num_passes=1, rollout_length_seconds=12 * 0.02, robot="kbot-headless", seed=5,
                        termination_params={"episode_length": {"max_length_sec": 25 * 0.02}})
    task = HumanoidWalkingTask(cfg)
    assert task.kcfg.max_episode_steps == 25 and task.kcfg.enable_randomizers == 1
    params = task.params.clone()
    perts = [RB.Perturbation("nominal"), RB.Perturbation("friction x0.25", friction_scale=0.25), RB.Perturbation("left leg torque x0.4", torque_scale={"left_leg": 0.4})]
    commands = [(), (0.6,)]
    kw = dict(perturbations=perts, commands=commands, repeats=2, seconds=1.0)
    entries, rec = task.robustness_sweep(**kw)
    dt = task.config.ctrl_dt
    ncases, N, T = 6, 12, 50
    aux, err, group, pert = rec.aux.cpu().numpy(), rec.err.cpu().numpy(), rec.group.cpu().numpy(), rec.pert.cpu().numpy()
    assert aux.shape == (T + 1, N, X["SIZE"]) and err.shape == (T, N, L.TERR["SIZE"]) and np.array_equal(group, np.arange(N) % ncases)
    assert np.array_equal(_bits(pert), _bits(np.stack([perts[(e % ncases) // 2].record() for e in range(N)])))
    done = aux[:T, :, X["DONE"]]
    assert (done[:T - 1] != 0).any(0).all(), "an env never restarted inside the run: the re-application behind a reset is not exercised"
    cmd = np.zeros((N, L.NCMD), np.float32)
    cmd[(np.arange(N) % ncases) % 2 == 1, 0] = 0.6
    assert np.array_equal(_bits(aux[:, :, X["CMD"]:X["CMD"] + L.NCMD]), _bits(np.tile(cmd, (T + 1, 1, 1))))       # every env held its command through the resets
    # the model rows after the last step: every env's record over whatever the last reset drew
    model = task.model_blob
    assert rec.ep.shape == (N, EP["SIZE"])
    assert np.array_equal(_bits(rec.ep), _bits(RR.perturbed_rows(model, pert, rec.ep)))                           # the written columns are the record's
    nominal_row = RR.perturbed_row(model, RR.identity_record(), rec.ep[0])
    mu, tl = np.float32(model.contact_mu), np.array(model.tau_limit, np.float32)
    for e in range(N):
        i = (e % ncases) // 2
        assert rec.ep[e, EP["MU"]] == (mu * np.float32(0.25) if i == 1 else mu)
        want_tl = tl.copy()
        if i == 2:
            want_tl[:5] = tl[:5] * np.float32(0.4)
        assert np.array_equal(rec.ep[e, EP["TAULIM"]:EP["ACTBIAS"]], want_tl) and np.array_equal(rec.ep[e, EP["KP"]:EP["KD"]], nominal_row[EP["KP"]:EP["KD"]])
    assert len(np.unique(rec.ep[:, EP["JPBIAS"]])) > 1                                                             # the sensor draws are each episode's own
    # the device's records and statistics
    want_rec, want = RR.robustness_ref(done, err, group, ncases)
    got_rec, got = rec.rec.cpu().numpy(), rec.stats.cpu().numpy()
    assert got_rec.dtype == np.float64 and RR.same_words(got_rec, want_rec) and RR.same_words(got, want)
    assert (got[:, S["ENVS"]] == 2).all() and (got[:, S["ROWS"]] == 2 * T).all() and (got[:, S["FALLS"]] + got[:, S["TIMEOUTS"]] >= 2).all()
    for c, x in enumerate(entries):
        i, j = c // 2, c % 2
        assert x["perturbation"] == perts[i].name and x["changed"] == perts[i].changed() and x["command"] == tuple(float(v) for v in cmd[c]) and x["mode"] == ("forward" if j else "stand")
        assert x["in_training_range"] == (i == 0) and (x["seconds"], x["repeats"]) == (T * dt, 2)
        for key, v in RB.case_summary(got[c], dt).items():
            assert _same(x[key], v), (c, key, x[key], v)
        assert x["envs"] == 2 and x["survival"] == 1 - got[c, S["FELL_ENVS"]] / 2 and x["falls_per_s"] == got[c, S["FALLS"]] / (2 * T * dt)
        assert x["settled_rows"] == got[c, S["SETTLED"]] and (x["settled_rows"] == 0 or x["lin_vel_err"] == got[c, S["ERR_SUM"]] / got[c, S["SETTLED"]])
    text = RB.format_robustness_table(entries)
    print(text)
    lines = text.splitlines()
    assert len(lines) == 2 + ncases and "not measured thresholds" in lines[0] and sum("*" in l for l in lines[2:]) == 4 and "xvel=+0.60" in text and "nan" not in text
    # a second call: the same bytes; the task itself is untouched
    entries2, rec2 = task.robustness_sweep(**kw)
    assert rec2.stats.cpu().numpy().tobytes() == got.tobytes() and rec2.rec.cpu().numpy().tobytes() == got_rec.tobytes()
    assert (task.params == params).all()
    # episodes of 25 rows never hold a command for the default 0.5 s: with a shorter settle time the error sums fill
    entries3, rec3 = task.robustness_sweep(settle_seconds=0.1, **kw)
    got3 = rec3.stats.cpu().numpy()
    want_rec3, want3 = RR.robustness_ref(rec3.aux.cpu().numpy()[:T, :, X["DONE"]], rec3.err.cpu().numpy(), group, ncases)
    assert RR.same_words(rec3.rec.cpu().numpy(), want_rec3) and RR.same_words(got3, want3) and (got3[:, S["SETTLED"]] > 0).all() and (got3[:, S["ERR_MAX"]] >= 0).all()
    assert all(x["settled_rows"] > 0 and x["lin_vel_err"] == got3[c, S["ERR_SUM"]] / got3[c, S["SETTLED"]] and x["settle"] == 5 * dt for c, x in enumerate(entries3))
    with pytest.raises(ValueError, match="torque_scale"):
        task.robustness_sweep(perturbations=[RB.Perturbation("bad", torque_scale=0.0)])
    with pytest.raises(ValueError, match="groups at most 256"):
        task.robustness_sweep(perturbations=[RB.Perturbation(f"p{k}") for k in range(65)], commands=[(), (0.1,), (0.2,), (0.3,)])
    task.close()
