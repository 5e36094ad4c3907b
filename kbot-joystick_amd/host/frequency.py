"""The command frequency response and its sweep: the Command term that moves one command word sinusoidally (SineCommand), the default
operating points and periods, the sweep behind HumanoidWalkingTask.frequency_sweep (one rollout, then ONE kbj_frequency_response call with
one group per case), what the host makes of the device's lock-in sums (gain, lag, delay, coherence, cross-coupling, the -3 dB bandwidth) and
its table. The rule of the sums is in include/kbj.h at kbj_frequency_response; everything in this file behind them is float64 host arithmetic.

The quadrature argument. The device sums the response y against the recorded command r and against d(t) = r(t - P / 4). For r = c + A cos(theta),
theta = 2 pi (t - s) / P, that is d = c + A cos(theta - pi / 2) = c + A sin(theta). Over whole periods the centred r and d are orthogonal and of
equal power, so the least-squares fit y ~ a (r - mean r) + b (d - mean d) + const of a response y = c' + g A cos(theta - phi) = c' + g A
(cos(phi) cos(theta) + sin(phi) sin(theta)) has a = g cos(phi), b = g sin(phi): gain g = hypot(a, b), lag phi = atan2(b, a), positive when
the response trails the stick. The 2 x 2 normal equations are solved as they are (not assumed diagonal): a sampled, fp32-rounded sinusoid
is orthogonal only within rounding."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ..spec import constants, layout as L
from . import binding as B
from .sweep import case_envs, command_label, command_table, held_command_rollout, steps_of, table_cell

R, S, O = L.FREC, L.FSTAT, L.FOUT
CHANNELS = constants.STEP_CHANNEL_NAMES
MIN_PERIOD, MAX_PERIOD = 4, 256          # kbj_frequency_response: a period is a multiple of 4 rows whose quarter fits the kernel's 64-row delay ring
DEFAULT_PERIODS = (200, 100, 48, 24, 12, 8)      # rows: 0.25, 0.5, 1.04, 2.08, 4.17 and 6.25 Hz at a 50 Hz control rate; round settings
BANDWIDTH_DB = -3.0


def sine_table(base_word, amp, period_rows) -> np.ndarray:
    """[N, max P] float32: entry [n, k] = base_word[n] + amp[n] cos(2 pi k / P[n]) for k < P[n], evaluated in float64 and rounded to fp32
    once; 0 behind an env's period."""
    base_word, amp, P = np.asarray(base_word, np.float64), np.asarray(amp, np.float64), np.asarray(period_rows, np.int64)
    k = np.arange(int(P.max()), dtype=np.float64)[None, :]
    value = base_word[:, None] + amp[:, None] * np.cos(2.0 * np.pi * k / P[:, None].astype(np.float64))
    return np.where(k < P[:, None], value, 0.0).astype(np.float32)


class SineCommand:
    """A Command term (train.py:724, 768) that moves ONE word of every env's command sinusoidally: env n holds its row of `base` [N, 16] with
    word `channel[n]` replaced by base + amp[n] cos(2 pi ((row - start_row) mod P[n]) / P[n]) (sine_table: float64, rounded to fp32 once); on
    the rows before `start_row` the word holds base + amp, the value of phase 0, so the sinusoid starts without a jump. Both
    `initial_command` and `__call__` answer by the row alone, so the schedule survives an in-episode reset, as SteppedCommand's does. The
    value depends on the row only through (row - start_row) mod P: the command a quarter period earlier is the same table a quarter
    period back, bit for bit."""

    def __init__(self, base: torch.Tensor, channel, amp, period_rows, start_row: int):
        self.base, self.start_row = base.to(torch.float32), int(start_row)
        dev = self.base.device
        ch, P = np.asarray(channel, np.int64), np.asarray(period_rows, np.int64)
        if ch.shape != (self.base.shape[0],) or P.shape != ch.shape or np.asarray(amp).shape != ch.shape:
            raise ValueError("SineCommand: channel, amp and period_rows have one value per env")
        if (ch < 0).any() or (ch >= L.NCMD).any() or (P < 1).any():
            raise ValueError("SineCommand: a channel is a command word and a period at least one row")
        self.channel, self.period = torch.from_numpy(ch).to(dev), torch.from_numpy(P).to(dev)
        self.envs = torch.arange(ch.shape[0], device=dev)
        base_word = self.base[self.envs, self.channel].cpu().numpy()
        self.table = torch.from_numpy(sine_table(base_word, amp, P)).to(dev)

    def scheduled(self, state):
        k = torch.remainder(max(int(state.row) - self.start_row, 0), self.period)
        out = self.base.clone()
        out[self.envs, self.channel] = self.table[self.envs, k]
        return out

    def initial_command(self, state, curriculum_level, rng):
        return self.scheduled(state)

    def __call__(self, prev_command, state, curriculum_level, rng):
        return self.scheduled(state)


def default_frequency_points(kcfg) -> list:
    """The sweep's default operating points (base command, channel, amplitude), from the command ranges of a kbj_config (train.py:1211-1217):
    each of the three channels around standing at half its range (half of the smaller of its two limits, so the stick stays inside them),
    and forward around half speed (0.5 vx_hi) at a quarter of its range (0.25 vx_hi). Round settings."""
    stand = (0.0,) * L.NCMD
    half = lambda lo, hi: 0.5 * min(abs(float(lo)), abs(float(hi)))
    return [(stand, 0, half(kcfg.vx_lo, kcfg.vx_hi)), (stand, 1, half(kcfg.vy_lo, kcfg.vy_hi)), (stand, 2, half(kcfg.wz_lo, kcfg.wz_hi)),
            ((0.5 * float(kcfg.vx_hi),) + (0.0,) * (L.NCMD - 1), 0, 0.25 * float(kcfg.vx_hi))]


def period_rows(value, ctrl_dt: float) -> int:
    """One entry of `periods` as a period in rows: an int is a period in rows, a float a frequency in Hz, snapped to
    P = 4 round(1 / (4 f ctrl_dt)). Refused: a period that is no multiple of 4 rows or outside [4, 256] (the device takes the quadrature
    reference a quarter period back, from a ring of 64 rows)."""
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        P = int(value)
        if P % 4:
            raise ValueError(f"frequency_sweep: a period of {P} rows is no multiple of 4 (the quadrature reference is the command a quarter period earlier)")
    else:
        f = float(value)
        if not f > 0 or not math.isfinite(f):
            raise ValueError(f"frequency_sweep: a frequency of {value!r} Hz")
        P = 4 * int(round(1.0 / (4.0 * f * ctrl_dt)))
    if P < MIN_PERIOD or P > MAX_PERIOD:
        raise ValueError(f"frequency_sweep: {value!r} is a period of {P} rows at ctrl_dt = {ctrl_dt:g} s; kbj_frequency_response takes periods in [{MIN_PERIOD}, {MAX_PERIOD}] rows "
                         f"({1.0 / (MAX_PERIOD * ctrl_dt):.3g} to {1.0 / (MIN_PERIOD * ctrl_dt):.3g} Hz: the kernel keeps 64 rows of the command per env)")
    return P


def case_schedule(P: int, ctrl_dt: float, cycles: int, min_window: float, start_row: int, settle_rows: int):
    """(s, K) of a case: K = max(cycles, ceil(min_window / (P ctrl_dt))) whole periods - min_window taken as round(min_window / ctrl_dt) rows,
    so the ceiling is one of whole numbers - from row s = start_row + ceil(settle_rows / P) P, a whole number of periods behind the start
    of the sinusoid (phase 0 on row s)."""
    K = max(int(cycles), -(-steps_of(min_window, ctrl_dt) // P))
    return start_row + -(-settle_rows // P) * P, K


@dataclasses.dataclass
class FrequencyRecord:
    """What a frequency sweep left on the device, for whoever wants more than the table: the aux rows [T + 1, N, AUX SIZE],
    kbj_frequency_response's signal [T, N, SSIG SIZE], its records [N, FREC SIZE] and group statistics [cases, FSTAT SIZE] (both float64), the
    schedule [N, 4] int32 (first measured row, period, channel, whole periods); env n belongs to case n % cases."""
    aux: torch.Tensor
    sig: torch.Tensor
    rec: torch.Tensor
    stats: torch.Tensor
    sched: torch.Tensor


def frequency_sweep(task, points=None, periods=None, cycles: int = 4, min_window: float = 4.0, start_at: float = 2.0, settle: float = 2.0,
                    min_amp=(0.05, 0.05, 0.05), repeats: int = 4, seed_offset: int = 7919):
    """The sweep behind HumanoidWalkingTask.frequency_sweep (see there): returns (entries, record) - one entry per case (operating point x
    period, the periods of a point in the order given), and the FrequencyRecord of what the run left on the device. Every call builds a
    context of its own and closes it again (host/sweep.py sweep_rollout)."""
    cfg = task.config
    dt = cfg.ctrl_dt
    points = default_frequency_points(task.kcfg) if points is None else list(points)
    plist = [period_rows(p, dt) for p in (DEFAULT_PERIODS if periods is None else periods)]
    if not points or not plist or repeats < 1 or cycles < 1:
        raise ValueError("frequency_sweep needs at least one operating point, one period, one cycle and one repeat")
    if any(len(pt) != 3 for pt in points):
        raise ValueError("frequency_sweep: an operating point is (base command, channel, amplitude)")
    base = command_table([pt[0] for pt in points], "frequency_sweep: the base command of operating point {i}")
    chan, amps = [int(pt[1]) for pt in points], [float(pt[2]) for pt in points]
    if any(not 0 <= c < L.NSCH for c in chan) or any(not a > 0 for a in amps):
        raise ValueError(f"frequency_sweep: a channel is one of {CHANNELS} (0, 1, 2) and an amplitude is positive")
    min_amp = [float(x) for x in min_amp]
    if len(min_amp) != L.NSCH:
        raise ValueError(f"frequency_sweep: min_amp has one value per channel {CHANNELS}")
    cases = [(i, P) for i in range(len(points)) for P in plist]
    start, settle_rows = steps_of(start_at, dt), steps_of(settle, dt)
    sk = [case_schedule(P, dt, cycles, min_window, start, settle_rows) for _, P in cases]
    for (_, P), (s, _) in zip(cases, sk):
        if s < P // 4:
            raise ValueError(f"frequency_sweep: start_at + settle puts the first measured row of the {P}-row period on row {s}; it needs {P // 4} rows (a quarter period) in front of it")
    ncases = len(cases)
    T = max(s + K * P for (_, P), (s, K) in zip(cases, sk))
    sched_c = np.array([[s, P, chan[i], K] for (i, P), (s, K) in zip(cases, sk)], np.int32)
    n, group, (base_env, sched) = case_envs(task, ncases, repeats, f"frequency_sweep: {ncases} cases, kbj_frequency_response", base[[i for i, _ in cases]], sched_c)
    dev = task.device                                                     # env e runs case e % ncases
    command = SineCommand(base_env, [chan[i] for i, _ in cases] * repeats, [amps[i] for i, _ in cases] * repeats, [P for _, P in cases] * repeats, start)
    with held_command_rollout(task, n, T, command, seed_offset) as (ctx, tr):
        crit = B.FrequencyCriteria((B.C.c_float * L.NSCH)(*min_amp))
        sig = torch.empty(T, n, L.SSIG["SIZE"], device=dev)
        rec = torch.empty(n, R["SIZE"], dtype=torch.float64, device=dev)
        stats = torch.empty(ncases, S["SIZE"], dtype=torch.float64, device=dev)
        ctx.frequency_response(tr.c, sched, crit, sig, rec, group, ncases, stats)
        ctx.synchronize()
        st = stats.cpu().numpy()
    settings = dict(start_at=start * dt, settle=settle_rows * dt, cycles=int(cycles), min_window=float(min_window), min_amp=tuple(min_amp), repeats=repeats)
    entries = [dict(point=i, base_command=tuple(float(x) for x in base[i]), channel=CHANNELS[chan[i]], amplitude=amps[i], period_rows=P, periods=sk[c][1], first_row=sk[c][0],
                    **settings, **case_summary(st[c], chan[i], P, dt)) for c, (i, P) in enumerate(cases)]
    for i in range(len(points)):
        mine = [e for e in entries if e["point"] == i]
        bw, below = bandwidth_hz([e["frequency_hz"] for e in mine], [e["gain_db"] for e in mine])
        for e in mine:
            e["bandwidth_hz"], e["bandwidth_below_range"] = bw, below
    return entries, FrequencyRecord(tr.aux, sig, rec, stats, sched)


def lockin(rows: float, sums, k: int) -> dict:
    """Channel k's response from `rows` and the 17 sums of a record or of a group's pooled statistics (layout.FREC order from S_R), float64:
    the centred products C_ab = S_AB - S_A S_B / rows; (a, b) solves [[C_rr, C_rd], [C_rd, C_dd]] (a, b) = (C_yr, C_yd); `gain` = hypot(a, b),
    `lag_rad` = atan2(b, a) (positive when the response trails the stick), `coherence` = (a C_yr + b C_yd) / C_yy, the share of the
    response's variance that is a linear copy of the input at that frequency. No rows or a singular system (a determinant that is not
    positive: the reference did not move) gives nan throughout; C_yy <= 0 (the response did not move) a nan coherence."""
    nan = float("nan")
    s = [float(x) for x in sums]
    n = float(rows)
    off = R["S_R"]
    sr, sd, srr, sdd, srd = (s[R[name] - off] for name in ("S_R", "S_D", "S_RR", "S_DD", "S_RD"))
    sy, syy, syr, syd = (s[R[name] - off + k] for name in ("S_Y", "S_YY", "S_YR", "S_YD"))
    if not n > 0:
        return dict(gain=nan, lag_rad=nan, coherence=nan)
    crr, cdd, crd = srr - sr * sr / n, sdd - sd * sd / n, srd - sr * sd / n
    cyy, cyr, cyd = syy - sy * sy / n, syr - sy * sr / n, syd - sy * sd / n
    det = crr * cdd - crd * crd
    if not det > 0 or not math.isfinite(det):
        return dict(gain=nan, lag_rad=nan, coherence=nan)
    a, b = (cyr * cdd - cyd * crd) / det, (cyd * crr - cyr * crd) / det
    return dict(gain=math.hypot(a, b), lag_rad=math.atan2(b, a), coherence=(a * cyr + b * cyd) / cyy if cyy > 0 else nan)


def case_summary(vec, channel: int, period: int, ctrl_dt: float) -> dict:
    """One KBJ_FSTAT vector (layout.FSTAT) of a case driven on `channel` with a period of `period` rows, as the figures of a table line:
    `frequency_hz` = 1 / (period ctrl_dt); `valid` windows (fell + measured + flat + censored) and the `void` count, each outcome's fraction
    of the valid ones, `fall_s_mean`; from the sums pooled over the MEASURED envs (lockin) `gain`, `gain_db` = 20 log10 gain, `lag_deg`,
    `delay_ms` = lag / (2 pi f), `coherence`, and per other channel `<ch>_coupling`, its gain against the same stick; `rows` measured and
    the command's `r_min` / `r_max`. A figure over nothing is nan."""
    vec = np.asarray(vec, np.float64)
    nan = float("nan")
    div = lambda a, b: float(a) / float(b) if b > 0 else nan
    cnt = {name: int(vec[S["COUNT"] + k]) for k, name in enumerate(constants.FREQUENCY_OUTCOME_NAMES)}
    valid = cnt["fell"] + cnt["measured"] + cnt["flat"] + cnt["censored"]
    f = 1.0 / (period * ctrl_dt)
    out = dict(frequency_hz=f, valid=valid, void=cnt["void"])
    for name in ("fell", "measured", "flat", "censored"):
        out[name + "_frac"] = div(cnt[name], valid)
    out["fall_s_mean"] = div(vec[S["FALL_SUM"]], cnt["fell"]) * ctrl_dt
    rows, sums = vec[S["ROWS"]], vec[S["SUMS"]:S["SUMS"] + L.FREC_NSUMS]
    own = lockin(rows, sums, channel)
    out.update(rows=int(rows), gain=own["gain"], gain_db=20.0 * math.log10(own["gain"]) if own["gain"] > 0 else (-math.inf if own["gain"] == 0 else nan),
               lag_deg=math.degrees(own["lag_rad"]), delay_ms=1e3 * own["lag_rad"] / (2.0 * math.pi * f), coherence=own["coherence"])
    for k, ch in enumerate(CHANNELS):
        if k != channel:
            out[ch + "_coupling"] = lockin(rows, sums, k)["gain"]
    out["r_min"], out["r_max"] = (float(vec[S["R_MIN"]]), float(vec[S["R_MAX"]])) if cnt["measured"] else (nan, nan)
    return out


def bandwidth_hz(freqs, gains_db, level: float = BANDWIDTH_DB):
    """(bandwidth in Hz, flagged): the frequency at which the gain first falls through `level` dB, by linear interpolation of the dB values
    over log f between the two measured frequencies that bracket the crossing (points whose gain is nan are left out). nan if the gain
    never crosses; if it is already below `level` at the lowest measured frequency, that frequency, flagged: the bandwidth lies below the
    range of the sweep."""
    pts = sorted((float(f), float(g)) for f, g in zip(freqs, gains_db) if g == g and f > 0)
    if not pts:
        return float("nan"), False
    if pts[0][1] < level:
        return pts[0][0], True
    for (f0, g0), (f1, g1) in zip(pts, pts[1:]):
        if g0 >= level > g1:
            if g1 == -math.inf:
                return f0, False
            x0, x1 = math.log(f0), math.log(f1)
            return math.exp(x0 + (level - g0) / (g1 - g0) * (x1 - x0)), False
    return float("nan"), False


def format_frequency_table(entries) -> str:
    """frequency_sweep's result as a text table: under a line that echoes the settings one line per case (the operating point by the
    non-zero components of its base command, the driven channel and amplitude, the frequency) - valid windows and voids, the outcome
    fractions of the valid ones, gain, gain in dB, lag in degrees, delay in ms, coherence and the larger of the two coupling gains ("-"
    over nothing) - then one bandwidth line per operating point."""
    def coupling(x):
        vals = [x[ch + "_coupling"] for ch in CHANNELS if ch + "_coupling" in x and x[ch + "_coupling"] == x[ch + "_coupling"]]
        return max(vals) if vals else float("nan")
    cols = (("hz", lambda x: x["frequency_hz"]), ("fell", lambda x: x["fell_frac"]), ("measured", lambda x: x["measured_frac"]), ("flat", lambda x: x["flat_frac"]),
            ("censored", lambda x: x["censored_frac"]), ("gain", lambda x: x["gain"]), ("gain_db", lambda x: x["gain_db"]), ("lag_deg", lambda x: x["lag_deg"]),
            ("delay_ms", lambda x: x["delay_ms"]), ("coherence", lambda x: x["coherence"]), ("coupling", coupling))
    label = lambda x: f"{command_label(x['base_command'])} {x['channel']} +-{x['amplitude']:.2f}"
    lines = []
    if entries:
        x = entries[0]
        amps = " ".join(f"{ch}>={a:g}" for ch, a in zip(CHANNELS, x["min_amp"]))
        lines.append(f"sinusoid from {x['start_at']:g} s, settle {x['settle']:g} s, at least {x['cycles']} periods and {x['min_window']:g} s measured, {x['repeats']} repeats; "
                     f"settings, not measured thresholds: command swing {amps}; linear-systems figures of a nonlinear walker: trust them as far as the coherence goes")
    labels = [label(x) for x in entries]
    w = max([len("operating point")] + [len(s) for s in labels])
    lines.append(f"{'operating point':{w}s}  {'P':>4s}  {'valid':>5s}  {'void':>4s}" + "".join(f"  {title:>10s}" for title, _ in cols))
    for s, x in zip(labels, entries):
        lines.append(f"{s:{w}s}  {x['period_rows']:4d}  {x['valid']:5d}  {x['void']:4d}" + "".join(table_cell(get(x)) for _, get in cols))
    seen = []
    for s, x in zip(labels, entries):
        if x["point"] in seen:
            continue
        seen.append(x["point"])
        bw = x.get("bandwidth_hz", float("nan"))
        text = "-" if bw != bw else f"{bw:.3f} Hz" + (" or lower: the gain is below it at the lowest frequency measured" if x.get("bandwidth_below_range") else "")
        lines.append(f"{s:{w}s}  {BANDWIDTH_DB:g} dB bandwidth: {text}")
    return "\n".join(lines)
