"""The command frequency response, the arithmetic that needs no GPU: what the synthetic set of tests/frequency_response_ref.py contains (the
condition that keeps tests/test_gpu_frequency_response.py from comparing nothing), the host formulas of host/frequency.py on a response whose
gain, lag and coherence are known in closed form, under a bound derived here from the rounding of the inputs, and the -3 dB interpolation on
a first-order lag's exact gains."""
import math

import numpy as np

from kbot_joystick_amd.host import frequency as F
from kbot_joystick_amd.spec import layout as L
from tests import frequency_response_ref as FR

G_, R, S, O = L.SSIG, L.FREC, L.FSTAT, L.FOUT
f32, f64 = np.float32, np.float64


def test_synthetic_set_contains_every_branch():
    prob = FR.problem()
    assert prob.aux.shape == (FR.T_SYN + 1, FR.N_SYN, L.AUX["SIZE"]) and prob.sched.shape == (FR.N_SYN, 4) and prob.sched.dtype == np.int32
    assert FR.N_SYN % 64 == 2 and FR.N_SYN > 128 and FR.T_SYN % 4 != 0 and FR.T_SYN >= 64 + 256
    c = FR.contents(prob)
    print(c)
    for name in ("NONE", "VOID", "FELL", "MEASURED", "FLAT", "CENSORED"):
        assert c[name] >= 5, (name, c[name])
    assert c["void_period"] >= 4 and c["void_channel"] >= 2 and c["void_cycles"] >= 1 and c["void_lead"] >= 1 and c["void_outside"] >= 2 and c["void_lead_done"] >= 5
    sched = prob.sched
    void_periods = {int(p) for p in sched[:, 1]}
    assert {0, 6, 260} <= void_periods and min(void_periods) < 0 and {-1, 3} <= {int(x) for x in sched[:, 2]} and 0 in sched[:, 3]
    assert (sched[:, 0] == FR.T_SYN).any() and (sched[:, 0] == FR.INT32_MAX).any()
    assert c["periods"] == [4, 8, 12, 64, 256] and {1, 3, FR.INT32_MAX} <= set(c["cycles"])
    assert c["fell_first"] >= 1 and c["fell_last"] >= 1 and c["timeout_first"] >= 1 and c["timeout_last"] >= 1
    assert c["by_T"] >= 10 and c["by_done"] >= 5 and c["on_amp"] >= 1 and c["nan_y"] >= 5 and c["nan_r"] >= 5 and c["nan_sums"] >= 10
    # a lead row on the first and on the last row of [s - q, s); the env with s == q is scanned
    rec, diag = FR.scan_ref(FR.device_like_signal(prob.aux, FR.T_SYN), sched, FR.MIN_AMP)
    n = next(n for n in range(FR.N_SYN) if sched[n, 1] == 64 and sched[n, 0] == 16)
    assert rec[n, R["OUTCOME"]] == O["MEASURED"] and rec[n, R["ROWS"]] == 192
    # the window that ends with the trajectory is whole; one row more and the trajectory cuts it
    whole = [n for n in range(FR.N_SYN) if int(sched[n, 0]) + int(sched[n, 1]) * int(sched[n, 3]) == FR.T_SYN and sched[n, 1] == 8]
    cut = [n for n in range(FR.N_SYN) if int(sched[n, 0]) + int(sched[n, 1]) * int(sched[n, 3]) == FR.T_SYN + 1 and sched[n, 1] == 8]
    assert whole and cut and all(rec[n, R["OUTCOME"]] == O["MEASURED"] for n in whole) and all(rec[n, R["OUTCOME"]] == O["CENSORED"] and diag[n]["by_T"] for n in cut)
    # NONE and VOID carry -1 everywhere else; FALL_STEPS is -1 unless FELL; the sums are kept for the outcomes that stopped early
    oc = rec[:, R["OUTCOME"]]
    assert (rec[oc <= O["VOID"], 1:] == -1).all() and (rec[(oc >= O["FELL"]) & (oc != O["FELL"]), R["FALL_STEPS"]] == -1).all()
    fell = oc == O["FELL"]
    assert (rec[fell, R["FALL_STEPS"]] == rec[fell, R["ROWS"]]).all() and (rec[fell, R["ROWS"]] == 0).any() and (rec[fell, R["ROWS"]] == 23).any()
    assert (rec[fell & (rec[:, R["ROWS"]] == 0), R["S_R"]:] == 0).all() and np.isinf(rec[fell & (rec[:, R["ROWS"]] == 0), R["R_MIN"]]).all()
    # the exact-swing envs are MEASURED, their neighbours one fp32 step below FLAT
    edge = [n for n in range(FR.N_SYN) if diag[n]["on_amp"]]
    assert edge and all(oc[n] == O["MEASURED"] and f32(rec[n, R["R_MAX"]]) - f32(rec[n, R["R_MIN"]]) == f32(FR.MIN_AMP[0]) for n in edge)
    # the statistics pool only MEASURED envs; envs 1 and 2 are in no group
    for G in (1, 3, 256):
        st = FR.group_stats_ref(rec, FR.groups(FR.N_SYN, G), G)
        assert st[:, S["COUNT"]:S["COUNT"] + O["COUNT"]].sum() == FR.N_SYN - 2
        keep = np.ones(FR.N_SYN, bool)
        keep[1:3] = False
        assert st[:, S["ROWS"]].sum() == rec[keep & (oc == O["MEASURED"]), R["ROWS"]].sum() and (st[:, S["R_MAX"] + 1:] == 0).all()
        empty = st[:, S["COUNT"] + O["MEASURED"]] == 0
        assert (st[empty, S["R_MIN"]] == -1).all() and (st[empty, S["R_MAX"]] == -1).all() and (G != 256 or empty.any())


def _sums_of(r, d, y):
    """(rows, the 17 sums) of fp32 samples r, d [n] and y [n, 3], as the device forms them."""
    r64, d64, y64 = r.astype(f64), d.astype(f64), y.astype(f64)
    s = [FR._ordered_sum(x) for x in (r64, d64, r64 * r64, d64 * d64, r64 * d64)]
    for block in (lambda k: y64[:, k], lambda k: y64[:, k] * y64[:, k], lambda k: y64[:, k] * r64, lambda k: y64[:, k] * d64):
        s += [FR._ordered_sum(block(k)) for k in range(3)]
    return len(r), np.array(s)


def test_known_gain_lag_and_coherence():
    """r = c_r + A cos(theta), d = r a quarter period earlier = c_r + A sin(theta), y = c + g A cos(theta - phi) + h cos(3 theta), all rounded to
    fp32, over K whole periods of P rows (P > 8: the third harmonic is orthogonal to the first on the sample grid). In exact arithmetic on the
    unrounded samples the centred r and d are orthogonal with C_rr = C_dd = C = n A^2 / 2, C_yr = g cos(phi) C, C_yd = g sin(phi) C and
    C_yy = n (g^2 A^2 + h^2) / 2: the formulas return g, phi and g^2 A^2 / (g^2 A^2 + h^2) exactly.
    The bound, from the inputs' rounding alone (u = 2^-24 relative per sample; nothing here is fitted to what the code returns):
      samples: |delta r|, |delta d| <= e_r = u (|c_r| + A), |delta y| <= e_y = u (|c| + g A + h); centring at most doubles a perturbation;
      the centred exact samples are bounded by A and by Y = g A + h.
      |dC_rr|, |dC_dd|, |dC_rd| <= n (4 A e_r + 4 e_r^2) + e64;  |dC_yr|, |dC_yd| <= n (2 Y e_r + 2 A e_y + 4 e_r e_y) + e64;
      |dC_yy| <= n (4 Y e_y + 4 e_y^2) + e64, with e64 = (n + 3) 2^-53 n max(|r|, |y|)^2 for the float64 adds and the S_A S_B / n cancellation.
      The system is (C I + dM)(x + dx) = v + dv with |x|_inf <= g and |dM|_inf <= m = 2 |dC_rr|: |da|, |db| <= e_ab = (|dC_yr| + m g) / (C - m).
      gain: hypot is 1-Lipschitz: |dg| <= sqrt(2) e_ab. lag: the angle of a vector moved by at most sqrt(2) e_ab: asin(sqrt(2) e_ab / g).
      coherence E / V: |dE| <= 2 (g |dC_yr| + e_ab (g C + |dC_yr|)), |dV| = |dC_yy|: |d(E / V)| <= (|dE| + |dV|) / (V - |dV|) as E <= V."""
    u = 2.0 ** -24
    worst = 0.0
    for P, K, c_r, A, c, g, phi, h in ((24, 3, 0.0, 0.6, 0.0, 0.8, 0.7, 0.0), (24, 3, 0.5, 0.3, 0.45, 0.5, 1.9, 0.1), (200, 4, 0.0, 0.5, -0.1, 1.2, -0.4, 0.05),
                                       (12, 5, 0.25, 0.25, 0.2, 0.05, 2.8, 0.02), (256, 1, 0.0, 1.0, 0.0, 0.3, 3.0, 0.3)):
        n, q = K * P, P // 4
        k = np.arange(-q, n)
        theta = 2.0 * np.pi * (k % P) / P
        r_all = (c_r + A * np.cos(theta)).astype(f32)
        r, d = r_all[q:], r_all[:-q]                                   # d(t) = r(t - q)
        th = theta[q:]
        y = np.zeros((n, 3), f32)
        y[:, 1] = (c + g * A * np.cos(th - phi) + h * np.cos(3.0 * th)).astype(f32)
        rows, sums = _sums_of(r, d, y)
        got = F.lockin(rows, sums, 1)
        e_r, e_y, Y = u * (abs(c_r) + A), u * (abs(c) + g * A + h), g * A + h
        e64 = (n + 3) * 2.0 ** -53 * n * max(abs(c_r) + A, abs(c) + Y) ** 2
        dcrr = n * (4 * A * e_r + 4 * e_r * e_r) + e64
        dcyr = n * (2 * Y * e_r + 2 * A * e_y + 4 * e_r * e_y) + e64
        dcyy = n * (4 * Y * e_y + 4 * e_y * e_y) + e64
        C, m = n * A * A / 2, 2 * dcrr
        e_ab = (dcyr + m * g) / (C - m)
        b_gain, b_lag = math.sqrt(2) * e_ab, math.asin(min(1.0, math.sqrt(2) * e_ab / g))
        E, V = g * g * C, n * (g * g * A * A + h * h) / 2
        b_coh = (2 * (g * dcyr + e_ab * (g * C + dcyr)) + dcyy) / (V - dcyy)
        assert b_gain < 1e-5 and b_lag < 1e-4 and b_coh < 1e-4, (b_gain, b_lag, b_coh)            # the bounds say something
        err = (abs(got["gain"] - g), abs(math.remainder(got["lag_rad"] - phi, 2 * math.pi)), abs(got["coherence"] - E / V))
        print(f"P={P} K={K}: gain {got['gain']:.9f} ({err[0]:.2e} of {b_gain:.2e}), lag {got['lag_rad']:.9f} ({err[1]:.2e} of {b_lag:.2e}), coherence {got['coherence']:.9f} ({err[2]:.2e} of {b_coh:.2e})")
        assert err[0] <= b_gain and err[1] <= b_lag and err[2] <= b_coh, (P, err, (b_gain, b_lag, b_coh))
        worst = max(worst, err[0] / b_gain, err[1] / b_lag, err[2] / b_coh)
        # the restatement's own formulas (numpy's solve) agree to float64 rounding of a well-conditioned 2 x 2 system
        ref = FR.response_ref(rows, sums, 1)
        assert abs(ref[0] - got["gain"]) <= 1e-12 and abs(ref[1] - got["lag_rad"]) <= 1e-12 and abs(ref[2] - got["coherence"]) <= 1e-12
        # the channels nobody drove: exactly zero response, so gain 0 and no coherence to speak of
        quiet = F.lockin(rows, sums, 0)
        assert quiet["gain"] == 0.0 and math.isnan(quiet["coherence"])
    print(f"largest error / bound {worst:.3f}")
    # nothing to solve: no rows, or a reference that did not move
    assert all(math.isnan(v) for v in F.lockin(0, np.zeros(17), 0).values())
    flat = _sums_of(np.full(16, 0.5, f32), np.full(16, 0.5, f32), np.ones((16, 3), f32))
    assert all(math.isnan(v) for v in F.lockin(*flat, 0).values()) and all(math.isnan(v) for v in FR.response_ref(*flat, 0))


def test_case_summary_units():
    """A response that trails a stick of 48 rows' period by exactly a quarter period (y = 0.5 d) at ctrl_dt = 0.02 s: 1 / 0.96 Hz, gain 0.5 =
    -6.02 dB, lag 90 degrees, delay 240 ms, coherence 1; within the float64 rounding of sums of exact fp32 products (the samples are
    multiples of 2^-3)."""
    P, K = 48, 2
    k = np.arange(-P // 4, K * P)
    tri = (np.abs(((k % P) / P) * 4.0 - 2.0) - 1.0)                    # a triangle wave in steps of 1 / 12: not fp32-exact, so scale to eighths
    r_all = (np.round(tri * 8) / 8).astype(f32)
    r, d = r_all[P // 4:], r_all[:-(P // 4)]
    y = np.zeros((K * P, 3), f32)
    y[:, 2] = f32(0.5) * d
    rows, sums = _sums_of(r, d, y)
    vec = np.zeros(S["SIZE"])
    vec[S["COUNT"] + O["MEASURED"]], vec[S["COUNT"] + O["FELL"]], vec[S["FALL_SUM"]] = 3, 1, 10
    vec[S["ROWS"]], vec[S["SUMS"]:S["SUMS"] + 17], vec[S["R_MIN"]], vec[S["R_MAX"]] = rows, sums, -1.0, 1.0
    x = F.case_summary(vec, 2, P, 0.02)
    assert abs(x["frequency_hz"] - 1.0 / 0.96) < 1e-12 and x["valid"] == 4 and x["void"] == 0 and x["measured_frac"] == 0.75 and x["fell_frac"] == 0.25
    assert abs(x["fall_s_mean"] - 0.2) < 1e-12 and x["rows"] == rows and (x["r_min"], x["r_max"]) == (-1.0, 1.0)
    assert abs(x["gain"] - 0.5) < 1e-12 and abs(x["gain_db"] - 20 * math.log10(0.5)) < 1e-10 and abs(x["lag_deg"] - 90.0) < 1e-9
    assert abs(x["delay_ms"] - 240.0) < 1e-6 and abs(x["coherence"] - 1.0) < 1e-12
    assert x["forward_coupling"] == 0.0 and x["sideways_coupling"] == 0.0 and "yaw_coupling" not in x


def test_bandwidth_interpolation():
    """A first-order lag, gain(f) = 1 / sqrt(1 + (f / fc)^2): the gain falls through -3 dB at f* = fc sqrt(10^0.3 - 1). With f* on the grid the
    interpolation returns it (to the rounding of a log and an exp). Between two grid points: dB over log f is concave for this gain (its slope
    falls from 0 to -20 dB per decade), so the chord lies below the curve and crosses -3 dB no later than the curve does: f_lo <= bw <= f*."""
    fc = 1.7
    db = lambda f: -10.0 * math.log10(1.0 + (f / fc) ** 2)
    fstar = fc * math.sqrt(10.0 ** 0.3 - 1.0)
    assert abs(db(fstar) + 3.0) < 1e-12
    grid = [0.25, 0.5, 1.0, fstar, 2.0, 4.0, 6.25]
    bw, below = F.bandwidth_hz(grid, [db(f) for f in grid])
    assert not below and abs(bw - fstar) <= 1e-12 * fstar
    grid = [6.25, 0.25, 2.08, 1.04, 0.5, 4.17]                         # unordered, as periods may be given
    bw, below = F.bandwidth_hz(grid, [db(f) for f in grid])
    assert not below and 1.04 <= bw <= fstar and bw < 2.08
    x0, x1 = math.log(1.04), math.log(2.08)
    assert abs(bw - math.exp(x0 + (-3.0 - db(1.04)) / (db(2.08) - db(1.04)) * (x1 - x0))) < 1e-12
    nan = float("nan")
    bw, below = F.bandwidth_hz([0.5, 1.04, 2.08], [db(0.5), nan, db(2.08)])      # a case without a measured gain is left out
    assert not below and 0.5 <= bw <= fstar
    bw, below = F.bandwidth_hz([0.25, 0.5, 1.0], [db(0.25), db(0.5), db(1.0)])   # never crosses
    assert math.isnan(bw) and not below
    bw, below = F.bandwidth_hz([2.08, 4.17], [db(2.08), db(4.17)])               # below -3 dB already at the lowest frequency: flagged
    assert bw == 2.08 and below
    bw, below = F.bandwidth_hz([1.0, 2.0], [nan, nan])
    assert math.isnan(bw) and not below
    assert F.bandwidth_hz([1.0, 2.0], [0.0, -math.inf]) == (1.0, False)          # a gain of exactly 0: no finite chord
