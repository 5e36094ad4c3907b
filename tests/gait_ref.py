"""Host restatement of kbj_gait_stats (include/kbj.h), in two parts: the scan as a plain loop per env - fp32 comparisons and fmaxf, float64 sums
in the stated order - that returns the statistics vector, the carry rows and the per-env record, and says which of the scan's rules fired; and
a deterministic generator of synthetic aux trajectories, two consecutive calls per shape, in which every rule is planted."""
import functools
import math

import numpy as np

from kbot_joystick_amd.spec import layout as L

G, F, A, E, X, M = L.GAIT, L.GFOOT, L.GACC, L.GENV, L.AUX, L.CMODE
f32 = np.float32
CONTACT_FORCE = f32(0.1)                         # rewards_kernel's contact test: TOUCH > 0.1f
FORCE_JUST_ABOVE = np.nextafter(CONTACT_FORCE, f32(1))
RUN_CAP = f32(2.0 ** 24)
CHUNK, ENVS = 4, 32                           # the kernel's chunk length (time steps) and envs per workgroup (csrc/kbj_gait_stats.h GAIT_TC, GAIT_ENVS)
# (T, N): the issue's four, then one below and one above a multiple of the chunk length with three and four chunks, N one above a multiple of
# the envs per workgroup (a staging buffer is used again, the last workgroup holds one env)
SHAPES = [(1, 1), (5, 63), (6, 64), (7, 65), (3 * CHUNK - 1, 2 * ENVS + 1), (3 * CHUNK + 1, ENVS + 1)]
REAL_SUMS = ("CLEAR_SUM", "CLEAR_SUMSQ", "FORCE_SUM")       # foot slots that are double sums of real values; TORQUE_SQ is the row slot
RULES = ("force_exactly_threshold_is_no_contact", "force_just_above_threshold_is_contact", "nan_force_is_no_contact", "touchdown_on_first_row_is_no_event",
         "first_phase_end_counted_without_duration", "phase_cut_by_failure", "phase_cut_by_timeout", "call_starts_an_episode_from_the_carry",
         "counted_phase_spans_the_call_boundary", "same_foot_twice_other_in_the_air", "flight_row", "double_support_row", "swing_below_stance_height_throughout",
         "mode_changes_in_mid_swing", "run_capped")


def mode_of(cmd) -> int:
    """KBJ_CMODE of one command (include/kbj.h kbj_tracking_stats)."""
    c = np.asarray(cmd, f32)
    nz, pose = c[:3] != 0, bool((c[3:] != 0).any())
    if not nz.any():
        return M["STAND_BEND"] if pose else M["STAND"]
    if pose or nz.sum() != 1:
        return M["OMNI"]
    return int(np.argmax(nz))


def slot(mode, name, foot=None):
    return L.gait_slot(mode, name, foot)


def gait_ref(acc, aux, T):
    """The scan of include/kbj.h kbj_gait_stats over rows 0 .. T-1 of aux [>= T, N, AUX SIZE] float32. `acc` [N, GACC SIZE] float32 is updated in
    place. Returns (stats, mags, env, fired): the KBJ_GAIT vector in float64 - counts, duration sums, sums of squares and maxima exact, the
    real-valued sums by math.fsum; per slot the sum of |x| of what a real-valued sum adds up (0 elsewhere); the per-env record [N, GENV SIZE]
    float32, its sums taken in float64 in row order and rounded once; and the set of RULES that fired."""
    N = aux.shape[1]
    stats, mags = np.zeros(G["SIZE"]), np.zeros(G["SIZE"])
    real = {}                                     # slot -> the values of a real-valued sum
    env = np.zeros((N, E["SIZE"]), f32)
    fired = set()

    def add_real(s, x):
        real.setdefault(s, []).append(float(x))

    for n in range(N):
        row = acc[n]
        con = [row[A["FOOT_STRIDE"] * f + A["CON"]] != 0 for f in range(2)]
        run = [f32(row[A["FOOT_STRIDE"] * f + A["RUN"]]) for f in range(2)]
        valid = [row[A["FOOT_STRIDE"] * f + A["VALID"]] != 0 for f in range(2)]
        zst = [f32(row[A["FOOT_STRIDE"] * f + A["ZST"]]) for f in range(2)]
        peak = [f32(row[A["FOOT_STRIDE"] * f + A["PEAK"]]) for f in range(2)]
        running, last_td = row[A["RUNNING"]] != 0, int(row[A["LAST_TD"]])
        touched = bool(run[0] != 0)               # the carry has seen a row before
        e = np.zeros(E["SIZE"])                   # this env's totals, float64
        # what only the fired table needs: the swing's lift-off mode, whether it stayed below the stance height, rows since the foot's last touchdown
        lift_mode, below, since_td = [None, None], [False, False], [None, None]
        for t in range(T):
            a = aux[t, n]
            Fc = [f32(a[X["TOUCH"] + f]) for f in range(2)]
            c = [bool(Fc[f] > CONTACT_FORCE) for f in range(2)]
            z = [f32(a[X["LFZ"]]), f32(a[X["RFZ"]])]
            mode = mode_of(a[X["CMD"]:X["CMD"] + L.NCMD])
            ctrl = a[X["CTRL"]:X["CTRL"] + L.NU]
            q, qmax = 0.0, f32(0)
            for u in range(L.NU):
                q += float(ctrl[u]) * float(ctrl[u])
                qmax = np.fmax(qmax, np.abs(f32(ctrl[u])))
            for f in range(2):
                if Fc[f] == CONTACT_FORCE and not c[f]:
                    fired.add("force_exactly_threshold_is_no_contact")
                if Fc[f] == FORCE_JUST_ABOVE and c[f]:
                    fired.add("force_just_above_threshold_is_contact")
                if np.isnan(Fc[f]) and not c[f]:
                    fired.add("nan_force_is_no_contact")
            # 1. the row
            support = ("FLIGHT", "SINGLE", "DOUBLE")[int(c[0]) + int(c[1])]
            if support == "FLIGHT":
                fired.add("flight_row")
            if support == "DOUBLE":
                fired.add("double_support_row")
            stats[slot(mode, "ROWS")] += 1; stats[slot(mode, support)] += 1
            add_real(slot(mode, "TORQUE_SQ"), q)
            stats[slot(mode, "TORQUE_MAX")] = max(stats[slot(mode, "TORQUE_MAX")], float(qmax))
            e[G["ROWS"]] += 1; e[G[support]] += 1; e[G["TORQUE_SQ"]] += q; e[G["TORQUE_MAX"]] = max(e[G["TORQUE_MAX"]], float(qmax))
            # 2. contact rows and ground force
            for f in range(2):
                if c[f]:
                    stats[slot(mode, "CONTACT_ROWS", f)] += 1
                    add_real(slot(mode, "FORCE_SUM", f), Fc[f])
                    stats[slot(mode, "FORCE_MAX", f)] = max(stats[slot(mode, "FORCE_MAX", f)], float(Fc[f]))
                    k = E["FOOT"] + E["FOOT_STRIDE"] * f + E["FORCE_MAX"]
                    e[k] = max(e[k], float(Fc[f]))
            if not running:        # 3. the row starts an episode
                stats[G["EPISODES"]] += 1
                if touched and t == 0:
                    fired.add("call_starts_an_episode_from_the_carry")
                for f in range(2):
                    if touched and not con[f] and c[f]:
                        fired.add("touchdown_on_first_row_is_no_event")
                    con[f], run[f], valid[f], zst[f], peak[f] = c[f], f32(1), False, z[f], f32(0)
                    lift_mode[f], below[f], since_td[f] = None, False, None
                last_td = -1
            else:                  # 4. phases and events
                for f in range(2):
                    if c[f] == con[f]:
                        if run[f] + f32(1) >= RUN_CAP:
                            fired.add("run_capped")
                        run[f] = np.minimum(f32(run[f] + f32(1)), RUN_CAP)
                        continue
                    r = float(run[f])
                    k = E["FOOT"] + E["FOOT_STRIDE"] * f
                    if not valid[f]:
                        fired.add("first_phase_end_counted_without_duration")
                    elif r > t:
                        fired.add("counted_phase_spans_the_call_boundary")
                    if c[f]:       # touchdown
                        stats[slot(mode, "TOUCHDOWNS", f)] += 1; e[k + E["TOUCHDOWNS"]] += 1
                        if valid[f]:
                            p = float(peak[f])
                            stats[slot(mode, "SWING_N", f)] += 1; stats[slot(mode, "SWING_SUM", f)] += r; stats[slot(mode, "SWING_SUMSQ", f)] += r * r
                            stats[slot(mode, "SWING_MAX", f)] = max(stats[slot(mode, "SWING_MAX", f)], r)
                            add_real(slot(mode, "CLEAR_SUM", f), p); add_real(slot(mode, "CLEAR_SUMSQ", f), p * p)
                            stats[slot(mode, "CLEAR_MAX", f)] = max(stats[slot(mode, "CLEAR_MAX", f)], p)
                            e[k + E["SWING_N"]] += 1; e[k + E["SWING_SUM"]] += r; e[k + E["CLEAR_SUM"]] += p; e[k + E["CLEAR_MAX"]] = max(e[k + E["CLEAR_MAX"]], p)
                            if below[f] and p == 0:
                                fired.add("swing_below_stance_height_throughout")
                            if lift_mode[f] is not None and lift_mode[f] != mode:
                                fired.add("mode_changes_in_mid_swing")
                        if last_td == f:
                            stats[slot(mode, "REPEATS")] += 1; e[G["REPEATS"]] += 1
                            o = 1 - f
                            if not con[o] and not c[o] and since_td[f] is not None and float(run[o]) >= since_td[f]:
                                fired.add("same_foot_twice_other_in_the_air")
                        last_td, since_td[f] = f, 0
                    else:          # lift-off
                        stats[slot(mode, "LIFTOFFS", f)] += 1
                        if valid[f]:
                            stats[slot(mode, "STANCE_N", f)] += 1; stats[slot(mode, "STANCE_SUM", f)] += r; stats[slot(mode, "STANCE_SUMSQ", f)] += r * r
                            stats[slot(mode, "STANCE_MAX", f)] = max(stats[slot(mode, "STANCE_MAX", f)], r)
                            e[k + E["STANCE_N"]] += 1; e[k + E["STANCE_SUM"]] += r
                        lift_mode[f], below[f] = mode, True
                    con[f], run[f], valid[f], peak[f] = c[f], f32(1), True, f32(0)
            # 5. the height of the last contact row, the rise over it
            for f in range(2):
                if c[f]:
                    zst[f] = z[f]
                else:
                    rise = f32(z[f] - zst[f])
                    peak[f] = np.fmax(peak[f], rise)
                    below[f] = below[f] and bool(rise < 0)
                if since_td[f] is not None:
                    since_td[f] += 1
            # 6.
            done = a[X["DONE"]]
            running = bool(done == 0)
            if done != 0 and (valid[0] or valid[1]):
                fired.add("phase_cut_by_failure" if done < 0 else "phase_cut_by_timeout")
            touched = True
        for f in range(2):
            b = A["FOOT_STRIDE"] * f
            row[b + A["CON"]], row[b + A["RUN"]], row[b + A["VALID"]], row[b + A["ZST"]], row[b + A["PEAK"]] = f32(con[f]), run[f], f32(valid[f]), zst[f], peak[f]
        row[A["RUNNING"]], row[A["LAST_TD"]] = f32(running), f32(last_td)
        env[n] = e.astype(f32)
    for s, xs in real.items():
        stats[s], mags[s] = math.fsum(xs), math.fsum(abs(x) for x in xs)
    return stats, mags, env, fired


def exact_slots():
    """The slots of a KBJ_GAIT vector that hold whole numbers or fp32 maxima: all but the real-valued sums."""
    m = np.ones(G["SIZE"], bool)
    for mode in range(M["COUNT"]):
        m[slot(mode, "TORQUE_SQ")] = False
        for f in range(2):
            for k in REAL_SUMS:
                m[slot(mode, k, f)] = False
    return m


def used_slots():
    m = np.zeros(G["SIZE"], bool)
    for mode in range(M["COUNT"]):
        m[mode * G["MODE_STRIDE"]:mode * G["MODE_STRIDE"] + 7] = True
        m[mode * G["MODE_STRIDE"] + G["FOOT"]:(mode + 1) * G["MODE_STRIDE"]] = True
    m[G["EPISODES"]] = True
    return m


def assert_stats_match(got, want, mags):
    """Counts, duration sums, sums of squares and maxima exact; the double sums of real values within 1e-9 * sum |x| of math.fsum (the margin
    tests/test_gpu_episode_stats.py derives for double accumulation in any order); unused slots 0."""
    ex = exact_slots()
    assert np.array_equal(got[ex], want[ex]), np.flatnonzero(ex)[got[ex] != want[ex]]
    assert (np.abs(got[~ex] - want[~ex]) <= 1e-9 * mags[~ex]).all(), (got[~ex], want[~ex])
    assert (got[~used_slots()] == 0).all()


# ---- synthetic problems ----
def _prototypes(rng):
    """One command per KBJ_CMODE, in mode order (the prototype vectors of train.py:744-749, with this env's magnitudes)."""
    vx, vy, wz, bh, rx, ry = rng.uniform(0.2, 1.0, 6) * rng.choice([-1.0, 1.0], 6)
    arms = np.where(rng.random(10) < 0.5, rng.uniform(-0.4, 0.4, 10), 0.0)
    z10 = np.zeros(10)
    rows = [[vx, 0, 0, 0, 0, 0, *z10], [0, vy, 0, 0, 0, 0, *z10], [0, 0, wz, 0, 0, 0, *z10], [vx, vy, wz, 0, 0, 0, *arms], [0, 0, 0, bh, rx, ry, *arms], [0.0] * 16]
    return np.array(rows, f32)


class Problems:
    """Two consecutive calls of one shape: `calls[i]` = aux [T + 1, N, 72] float32 of call i (row T is never read: it holds 1e9), `acc0` the
    carry the first call starts from: zeros, the spare floats 7.0, and env 1's planted phase. Every column the kernel does not read holds
    noise. Every env follows a random contact pattern (phases of 1-4 rows, episode ends on 8 % of the rows, a command of each mode by turns,
    changed now and then); with T >= 5 and N >= 8 the first envs are scripted instead, over the 2 T rows r of both calls:
      env 0: foot 0's force is exactly 0.1f on row 1 (no contact) and NaN on row 2; foot 1's is nextafter(0.1f, 1) on row 1 (contact).
      env 1: carry RUNNING, foot 0 in a counted stance with RUN = 2^24 - 1; three more rows of it, then the foot lifts: a stance of 2^24 rows.
      env 2: both feet down, foot 0 lifts on row 1 (the first phase: its end counts, its duration does not), DONE = -1 on row 2 cuts the swing;
             row 3 starts an episode with foot 0 down again (no touchdown event); foot 1 lifts on row T - 1, where DONE = +1 cuts that swing and
             makes call 2 start an episode.
      env 3: foot 1 in the air throughout; foot 0 down on row 0, up on 1, down on 2, up on 3, down again on row T + 1 (a swing of T - 2 rows
             over the call boundary), up on T + 2, down on T + 3: the same foot touching down twice. Rows 1 and 3 .. T are flight rows.
      env 4: both feet down at 0.10 m; foot 0 swings on rows 1 and 2 BELOW that height (clearance 0) while the command goes from forward to
             sideways on row 2; it touches down on row 3, in the sideways block."""

    def __init__(self, T, N):
        rng = np.random.default_rng(1000 * T + N)
        R = 2 * T
        c = np.zeros((R, N, 2), bool)
        z = np.zeros((R, N, 2), f32)
        done = np.where(rng.random((R, N)) < 0.08, rng.choice([-1.0, 1.0], (R, N)), 0.0).astype(f32)
        cmd = np.zeros((R, N, L.NCMD), f32)
        for n in range(N):
            protos = _prototypes(rng)
            mode, r = (n + int(rng.integers(0, 2))) % M["COUNT"], 0
            while r < R:
                hold = int(rng.integers(2, R + 2))
                cmd[r:r + hold, n] = protos[mode]
                mode, r = int(rng.integers(0, M["COUNT"])), r + hold
            for f in range(2):
                r, down = 0, bool(rng.integers(0, 2))
                while r < R:
                    d = int(rng.integers(1, 5))
                    c[r:r + d, n, f] = down
                    down, r = not down, r + d
            z[:, n] = np.where(c[:, n], rng.uniform(0.02, 0.06, (R, 2)), rng.uniform(0.0, 0.2, (R, 2)))
        planted = T >= 5 and N >= 8
        if planted:
            protos = _prototypes(rng)
            c[:, :5], done[:, :5], cmd[:, :5] = True, 0.0, protos[M["FORWARD"]]
            cmd[:, 1], cmd[:, 3] = protos[M["OMNI"]], protos[M["STAND_BEND"]]
            z[:, :5] = f32(0.04)
            c[3:, 1, 0] = False
            c[1:3, 2, 0], done[2, 2], c[T - 1:T + 2, 2, 1], done[T - 1, 2] = False, -1.0, False, 1.0
            c[:, 3, 1], c[:, 3, 0] = False, False
            c[0, 3, 0] = c[2, 3, 0] = True
            c[T + 1:, 3, 0], c[T + 2, 3, 0] = True, False
            z[:, 3] = np.where(c[:, 3], f32(0.04), f32(0.04) + rng.uniform(0.01, 0.1, (R, 2)).astype(f32))
            z[:, 4, 0], c[1:3, 4, 0], cmd[2:, 4] = f32(0.10), False, protos[M["SIDEWAYS"]]
            z[1, 4, 0], z[2, 4, 0] = f32(0.05), f32(0.08)
        force = np.where(c, rng.uniform(20.0, 400.0, (R, N, 2)), rng.choice([0.0, 0.05, -1.0], (R, N, 2))).astype(f32)
        if planted:
            force[1, 0, 0], force[1, 0, 1], force[2, 0, 0] = CONTACT_FORCE, FORCE_JUST_ABOVE, np.nan
        aux = rng.standard_normal((R, N, X["SIZE"])).astype(f32)
        aux[:, :, X["TOUCH"]:X["TOUCH"] + 2], aux[:, :, X["LFZ"]], aux[:, :, X["RFZ"]] = force, z[:, :, 0], z[:, :, 1]
        aux[:, :, X["CTRL"]:X["CTRL"] + L.NU] = (rng.standard_normal((R, N, L.NU)) * rng.uniform(1.0, 40.0, (R, N, 1))).astype(f32)
        aux[:, :, X["CMD"]:X["CMD"] + L.NCMD], aux[:, :, X["DONE"]] = cmd, done
        self.T, self.N, self.planted = T, N, planted
        self.calls = [np.concatenate([aux[i * T:(i + 1) * T], np.full((1, N, X["SIZE"]), 1e9, f32)]) for i in range(2)]
        self.acc0 = np.zeros((N, A["SIZE"]), f32)
        self.acc0[:, [A["FOOT_STRIDE"] - 1, 2 * A["FOOT_STRIDE"] - 1, A["LAST_TD"] + 1, A["LAST_TD"] + 2]] = 7.0
        if planted:
            self.acc0[1, [A["CON"], A["RUN"], A["VALID"], A["ZST"]]] = (1.0, 2.0 ** 24 - 1, 1.0, 0.04)
            self.acc0[1, [A["FOOT_STRIDE"] + A["CON"], A["FOOT_STRIDE"] + A["RUN"], A["FOOT_STRIDE"] + A["VALID"], A["FOOT_STRIDE"] + A["ZST"]]] = (1.0, 5.0, 1.0, 0.04)
            self.acc0[1, A["RUNNING"]], self.acc0[1, A["LAST_TD"]] = 1.0, 0.0


@functools.lru_cache(maxsize=None)
def problems(T, N):
    return Problems(T, N)


@functools.lru_cache(maxsize=None)
def reference(T, N):
    """The restatement on both calls of problems(T, N), computed once: a list of (acc before, acc after, stats, mags, env, fired) per call. Shared
    by the tests; nobody writes to it."""
    P = problems(T, N)
    acc, out = P.acc0.copy(), []
    for aux in P.calls:
        before = acc.copy()
        stats, mags, env, fired = gait_ref(acc, aux, T)
        out.append((before, acc.copy(), stats, mags, env, fired))
    return out
