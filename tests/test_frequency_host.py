"""The command frequency response, the host parts that need no GPU: the layout mirrors against include/kbj_model.h, the SineCommand term through
UserTerms.apply_command against a context that records its calls (its rows bit for bit the formula's, its quarter-period shift exact for
every default period, its survival of in-episode resets), frequency snapping and the refusals, K and s per case, the default operating
points, the summary and the table on hand-made statistics."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

from kbot_joystick_amd.host import frequency as F
from kbot_joystick_amd.spec import compiler, constants, layout as L
from tests.test_step_host import _Recorder, _Rows      # the Context stand-in that records kbj_env_set_command, and bare trajectory rows

R, S, O, X = L.FREC, L.FSTAT, L.FOUT, L.AUX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_layout_mirrors_the_header():
    assert L.FREC_NSUMS == R["SIZE"] - R["S_R"] == 17                # (values against the header: tests/test_abi_mirror.py)
    assert [O[n.upper()] for n in constants.FREQUENCY_OUTCOME_NAMES] == list(range(O["COUNT"]))
    assert O["FELL"] == L.SOUT["FELL"] and O["CENSORED"] == L.SOUT["CENSORED"] and min(O[k] for k in ("FELL", "MEASURED", "FLAT", "CENSORED")) == O["FELL"]
    assert R["S_Y"] + L.NSCH == R["S_YY"] and R["S_YY"] + L.NSCH == R["S_YR"] and R["S_YR"] + L.NSCH == R["S_YD"] and R["S_YD"] + L.NSCH == R["SIZE"]
    assert (2 * R["SIZE"]) % 4 == 0                                  # a record of doubles is staged as 16-byte pieces of floats
    assert S["COUNT"] + O["COUNT"] == S["FALL_SUM"] and S["SUMS"] + L.FREC_NSUMS == S["R_MIN"] and S["R_MAX"] < S["SIZE"]
    from kbot_joystick_amd.host import binding
    assert ctypes.sizeof(binding.FrequencyCriteria) == 4 * L.NSCH == binding.load_library().kbj_sizeof_frequency_criteria()
    kbj = open(os.path.join(ROOT, "include", "kbj.h")).read()
    for text in ("float min_amp[3];", "int kbj_frequency_response(kbj_ctx* ctx", "K * P in particular"):
        assert text in kbj, text
    assert "No sine or cosine is\n * evaluated on the device" in kbj and "SETTING of the caller, not a measured" in kbj
    assert "kbj_frequency_response" in binding.SIGNATURES and "kbj_sizeof_frequency_criteria" in binding.SIGNATURES
    assert F.MAX_PERIOD == 256 and F.MIN_PERIOD == 4 and all(P % 4 == 0 and F.MIN_PERIOD <= P <= F.MAX_PERIOD for P in F.DEFAULT_PERIODS)
    assert F.DEFAULT_PERIODS == (200, 100, 48, 24, 12, 8)


def _formula(base_word, amp, P, k):
    """base + amp cos(2 pi k / P): float64, rounded to fp32 once."""
    return f32(np.float64(f32(base_word)) + np.float64(amp) * math.cos(2.0 * math.pi * k / P))


def test_sine_command_rows():
    """Rows 0 .. 40 of four envs, the sinusoid from row 5: periods 8, 12, 24 and 4 on the channels 0, 1, 2, 0. Env 1's episode ends in step 6
    (fresh on row 7), env 2's in step 20: the kernel's reset has put the context's fixed command (here 9s) into their rows, and the term
    writes the scheduled command again. Every row of every env holds the formula's fp32 value, bit for bit; the other 15 words hold the base."""
    from kbot_joystick_amd.host.user_terms import UserTerms
    T, N, start = 40, 4, 5
    tr, ctx = _Rows(T, N), _Recorder()
    tr.aux[:, :, X["BQUAT"]] = 1.0
    tr.aux[6, 1, X["DONE"]], tr.aux[20, 2, X["DONE"]] = -1.0, 1.0
    tr.aux[7, 1, X["CMD"]:X["CMD"] + L.NCMD] = 9.0
    tr.aux[21, 2, X["CMD"]:X["CMD"] + L.NCMD] = 9.0
    base = torch.zeros(N, L.NCMD)
    base[3, 0], base[:, 3] = 0.6, 0.125
    chan, amp, P = [0, 1, 2, 0], [0.6, 0.25, 0.5, 0.3], [8, 12, 24, 4]
    terms = UserTerms(command=F.SineCommand(base, chan, amp, P, start))
    terms.bind(5, 0, torch.device("cpu"), compiler.load_model("kbot-headless"), L.NOBS_ACTOR, L.NOBS_CRITIC)
    for row in range(T + 1):
        terms.run_hooks(ctx, tr, row, 100 + row, [terms.apply_command])
    assert len(ctx.calls) == T + 1
    for row, cmd in enumerate(ctx.calls):
        want = base.clone().numpy()
        for n in range(N):
            want[n, chan[n]] = _formula(base[n, chan[n]].item(), amp[n], P[n], (row - start) % P[n] if row >= start else 0)
        assert np.array_equal(cmd.numpy().view(np.uint32), want.view(np.uint32)), row
        assert np.array_equal(tr.aux[row, :, X["CMD"]:X["CMD"] + L.NCMD].numpy().view(np.uint32), want.view(np.uint32)), row
    # before the start the word holds base + amp, the value the sinusoid starts from: no jump on row `start`
    assert all(ctx.calls[r][3, 0].item() == _formula(0.6, 0.3, 4, 0) for r in range(start + 1)) and ctx.calls[start + 1][0, 0] < ctx.calls[start][0, 0]
    with pytest.raises(ValueError, match="one value per env"):
        F.SineCommand(base, [0, 1], amp, P, 0)
    with pytest.raises(ValueError, match="a command word"):
        F.SineCommand(base, [0, 1, 2, 16], amp, P, 0)


def test_quarter_period_shift_is_exact():
    """The device takes d(t) = r(t - P / 4) from the recorded rows. SineCommand's value depends on the row only through (row - start) mod P, so
    for every default period the row a quarter period earlier is the same table entry a quarter period back - bit for bit, over several
    periods - and that entry is the sine the quadrature argument asks for, c + A sin(theta), within the rounding of the fp32 result and of
    the float64 cosine's argument (half an fp32 ulp of the largest value plus 4 x 2^-53 x 2 pi A)."""
    start, base_word, A = 3, 0.25, 0.5
    for P in F.DEFAULT_PERIODS:
        q = P // 4
        base = torch.zeros(1, L.NCMD)
        base[0, 1] = base_word
        term = F.SineCommand(base, [1], [A], [P], start)
        rows = [term.scheduled(types.SimpleNamespace(row=row))[0, 1].item() for row in range(start + 3 * P + 1)]
        table = F.sine_table([base_word], [A], [P])[0]
        assert table.dtype == np.float32 and len(table) == P
        for row in range(start + q, len(rows)):
            k = (row - start) % P
            assert f32(rows[row]) == table[k] and f32(rows[row - q]) == table[(k - q) % P], (P, row)
            bound = 0.5 * np.spacing(f32(abs(base_word) + A)) + 4 * 2.0 ** -53 * 2 * math.pi * A
            assert abs(rows[row - q] - (base_word + A * math.sin(2.0 * math.pi * k / P))) <= bound, (P, row)


def test_periods_frequencies_and_schedule():
    dt = 0.02
    assert [F.period_rows(P, dt) for P in F.DEFAULT_PERIODS] == list(F.DEFAULT_PERIODS)
    # a frequency in Hz snaps to P = 4 round(1 / (4 f dt))
    assert F.period_rows(1.0, dt) == 48 and F.period_rows(0.25, dt) == 200 and F.period_rows(2.0, dt) == 24 and F.period_rows(6.25, dt) == 8
    assert F.period_rows(12.5, dt) == 4 and F.period_rows(0.21, dt) == 240 and F.period_rows(np.int64(12), dt) == 12 and F.period_rows(3.0, dt) == 16
    for bad, why in ((6, "no multiple of 4"), (0, r"period of 0 rows .* \[4, 256\]"), (260, r"period of 260 rows .* \[4, 256\]"), (-8, r"\[4, 256\]"),
                     (0.1, r"period of 500 rows .* \[4, 256\]"), (40.0, r"period of 0 rows"), (0.0, "frequency"), (-1.0, "frequency"), (float("nan"), "frequency")):
        with pytest.raises(ValueError, match=why):
            F.period_rows(bad, dt)
    # K = max(cycles, ceil(min_window / (P dt))) whole periods; s = start + ceil(settle_rows / P) P
    want = {200: (300, 4), 100: (200, 4), 48: (244, 5), 24: (220, 9), 12: (208, 17), 8: (204, 25)}
    for P, (s, K) in want.items():
        assert F.case_schedule(P, dt, 4, 4.0, 100, 100) == (s, K), P
        assert K * P * dt >= 4.0 - 1e-9 and (K == 4 or (K - 1) * P * dt < 4.0) and (s - 100) % P == 0 and 100 <= s - 100 < 100 + P
    assert F.case_schedule(24, dt, 4, 1.0, 3, 3) == (27, 4) and F.case_schedule(8, dt, 4, 1.0, 3, 3) == (11, 7) and F.case_schedule(8, dt, 2, 0.0, 5, 0) == (5, 2)


def test_default_operating_points():
    k = L.default_config()
    pts = F.default_frequency_points(k)
    assert len(pts) == 4 and all(len(p[0]) == L.NCMD for p in pts) and [p[1] for p in pts] == [0, 1, 2, 0]
    assert all(v == 0 for p in pts[:3] for v in p[0]) and pts[3][0][0] == pytest.approx(0.5 * k.vx_hi) and all(v == 0 for v in pts[3][0][1:])
    assert pts[0][2] == pytest.approx(0.5 * min(k.vx_hi, -k.vx_lo)) and pts[1][2] == pytest.approx(0.5 * k.vy_hi) and pts[2][2] == pytest.approx(0.5 * k.wz_hi)
    assert pts[3][2] == pytest.approx(0.25 * k.vx_hi)
    for base, ch, amp in pts:                                          # the stick stays inside the command ranges
        lo, hi = ((k.vx_lo, k.vx_hi), (k.vy_lo, k.vy_hi), (k.wz_lo, k.wz_hi))[ch]
        assert lo - 1e-6 <= base[ch] - amp and base[ch] + amp <= hi + 1e-6


def test_sweep_refuses_what_the_kernel_cannot_take():
    task = types.SimpleNamespace(config=types.SimpleNamespace(ctrl_dt=0.02), kcfg=L.default_config())
    stand = (0.0,)
    with pytest.raises(ValueError, match=r"period of 260 rows .* \[4, 256\]"):
        F.frequency_sweep(task, periods=[260])
    with pytest.raises(ValueError, match=r"0.195 to 12.5 Hz"):
        F.frequency_sweep(task, periods=[0.1])
    with pytest.raises(ValueError, match="no multiple of 4"):
        F.frequency_sweep(task, periods=[10])
    with pytest.raises(ValueError, match="at most 256"):
        F.frequency_sweep(task, points=[(stand, 0, 0.5)] * 65, periods=[8, 12, 24, 48])
    with pytest.raises(ValueError, match="at least one operating point"):
        F.frequency_sweep(task, points=[])
    with pytest.raises(ValueError, match="at least one operating point"):
        F.frequency_sweep(task, periods=[])
    with pytest.raises(ValueError, match=r"\(base command, channel, amplitude\)"):
        F.frequency_sweep(task, points=[(stand, 0)])
    with pytest.raises(ValueError, match="a channel is one of"):
        F.frequency_sweep(task, points=[(stand, 3, 0.5)])
    with pytest.raises(ValueError, match="amplitude is positive"):
        F.frequency_sweep(task, points=[(stand, 0, 0.0)])
    with pytest.raises(ValueError, match="17 components"):
        F.frequency_sweep(task, points=[((0.0,) * 17, 0, 0.5)])
    with pytest.raises(ValueError, match="one value per channel"):
        F.frequency_sweep(task, min_amp=(0.1, 0.1))
    with pytest.raises(ValueError, match=r"needs 50 rows \(a quarter period\) in front"):
        F.frequency_sweep(task, periods=[200], start_at=0.5, settle=0.0)


def _vec(measured, rows, sums, **counts):
    vec = np.zeros(S["SIZE"])
    vec[S["COUNT"] + O["MEASURED"]] = measured
    for name, v in counts.items():
        vec[S["COUNT"] + O[name.upper()]] = v
    vec[S["ROWS"]], vec[S["SUMS"]:S["SUMS"] + L.FREC_NSUMS] = rows, sums
    vec[S["R_MIN"]], vec[S["R_MAX"]] = (-0.5, 0.5) if measured else (-1.0, -1.0)
    return vec


def test_case_summary_and_table():
    """Hand-made pooled sums over 2 x 8 rows of P = 8: r = cos, d = sin (sampled, float64), y_forward = 0.5 r + 0.5 d (gain 1 / sqrt 2 = -3.01 dB,
    lag 45 degrees = a delay of 20 ms at 6.25 Hz, coherence 1), y_yaw = 0.1 r (a coupling gain of 0.1), y_sideways = 0."""
    P, n = 8, 16
    th = 2.0 * np.pi * (np.arange(n) % P) / P
    r, d = 0.5 * np.cos(th), 0.5 * np.sin(th)
    y = np.stack([0.5 * r + 0.5 * d, np.zeros(n), 0.1 * r], axis=1)
    sums = [r.sum(), d.sum(), (r * r).sum(), (d * d).sum(), (r * d).sum()]
    for f in (lambda k: y[:, k], lambda k: y[:, k] ** 2, lambda k: y[:, k] * r, lambda k: y[:, k] * d):
        sums += [f(k).sum() for k in range(3)]
    x = F.case_summary(_vec(2, n, sums, void=1, fell=1, censored=1), 0, P, 0.02)
    assert (x["valid"], x["void"], x["fell_frac"], x["measured_frac"], x["flat_frac"], x["censored_frac"]) == (4, 1, 0.25, 0.5, 0.0, 0.25)
    assert x["frequency_hz"] == pytest.approx(6.25) and x["rows"] == 16 and (x["r_min"], x["r_max"]) == (-0.5, 0.5)
    assert x["gain"] == pytest.approx(math.sqrt(0.5), abs=1e-12) and x["gain_db"] == pytest.approx(-3.0103, abs=1e-4) and x["lag_deg"] == pytest.approx(45.0, abs=1e-9)
    assert x["delay_ms"] == pytest.approx(20.0, abs=1e-9) and x["coherence"] == pytest.approx(1.0, abs=1e-12)
    assert x["yaw_coupling"] == pytest.approx(0.1, abs=1e-12) and x["sideways_coupling"] == 0.0 and "forward_coupling" not in x
    empty = F.case_summary(_vec(0, 0, np.zeros(17), void=4), 0, P, 0.02)
    assert empty["valid"] == 0 and empty["void"] == 4 and empty["rows"] == 0
    assert all(math.isnan(v) for k, v in empty.items() if k not in ("valid", "void", "rows", "frequency_hz"))
    settings = dict(start_at=2.0, settle=2.0, cycles=4, min_window=4.0, min_amp=(0.05, 0.05, 0.1), repeats=4)
    z = (0.0,) * 16
    low = dict(x, frequency_hz=1.0 / (24 * 0.02), gain=1.0, gain_db=0.0)
    entries = [dict(point=0, base_command=z, channel="forward", amplitude=0.6, period_rows=24, bandwidth_hz=5.5, bandwidth_below_range=False, **settings, **low),
               dict(point=0, base_command=z, channel="forward", amplitude=0.6, period_rows=8, bandwidth_hz=5.5, bandwidth_below_range=False, **settings, **x),
               dict(point=1, base_command=(0.6,) + z[1:], channel="yaw", amplitude=0.5, period_rows=8, bandwidth_hz=float("nan"), bandwidth_below_range=False, **settings, **empty),
               dict(point=2, base_command=z, channel="sideways", amplitude=0.25, period_rows=8, bandwidth_hz=6.25, bandwidth_below_range=True, **settings, **x)]
    text = F.format_frequency_table(entries)
    print(text)
    lines = text.splitlines()
    assert len(lines) == 1 + 1 + 4 + 3 and "settings, not measured thresholds" in lines[0] and "yaw>=0.1" in lines[0] and "coherence" in lines[0]
    assert lines[2].startswith("(zero) forward +-0.60") and lines[2].split()[3:8] == ["24", "4", "1", "2.083", "0.250"]
    assert lines[3].split()[3:6] == ["8", "4", "1"] and "-3.010" in lines[3] and "45.000" in lines[3] and "20.000" in lines[3]
    assert lines[4].startswith("xvel=+0.60 yaw +-0.50") and " - " in lines[4] + " " and "nan" not in text
    assert lines[6].startswith("(zero) forward +-0.60") and lines[6].endswith("-3 dB bandwidth: 5.500 Hz")
    assert lines[7].endswith("-3 dB bandwidth: -") and "6.250 Hz or lower" in lines[8]
    assert F.format_frequency_table([]).count("\n") == 0
    # the bandwidth of the first operating point from its two cases, as frequency_sweep attaches it
    bw, below = F.bandwidth_hz([e["frequency_hz"] for e in entries[:2]], [e["gain_db"] for e in entries[:2]])
    assert not below and 1.0 / 0.48 < bw < 6.25 and bw == pytest.approx(6.25, rel=5e-3)      # -3.0103 dB at 6.25 Hz: the crossing lies just below it
