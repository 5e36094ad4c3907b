"""Host restatement of kbj_tracking_stats (include/kbj.h), in three parts: the five errors of an aux row in float64; the same in float32 in
rewards_kernel's operation order (`errors(..., np.float32)`: what separates the two is the spread S_k the GPU bound is built from); the
mode rule and the settle scan as plain loops, with the statistics by math.fsum. And the synthetic problems that
tests/test_tracking_host.py checks conditions on and tests/test_gpu_tracking_stats.py runs through the ABI."""
import functools
import math

import numpy as np

from kbot_joystick_amd.spec import layout as L

K, A, R, X, M = L.TRK, L.TACC, L.TERR, L.AUX, L.CMODE
NE = L.NTERR
SHAPES = [(1, 1), (7, 65), (8, 96), (5, 130)]      # a lone env; ragged last blocks of 1 and of 32 envs; more than two blocks
CALLS = 3                                          # chained calls per shape, so that the carry matters
STANDARD_HEIGHT, FOOT_ORIGIN_HEIGHT = 0.80, 0.06   # layout.default_config's rew_standard_height / rew_foot_origin_height


# ---- part 1 and 2: the five errors, in `dtype` arithmetic ----
def errors(aux, joint_bias, standard_height, foot_origin_height, dtype=np.float64):
    """aux [..., 72] float32 -> (err [..., 5], mag [5]) in `dtype`: rewards_kernel's expressions before their exp (kbj_traj_stats.hip; quat_to_euler,
    euler_to_quat, rotate_by_quat of kbj_env_core.h), operation by operation. mag[k] = the largest operand magnitude of expression k."""
    f = dtype
    a = np.asarray(aux, np.float32).astype(f)
    one, two = f(1), f(2)
    cmd = a[..., X["CMD"]:X["CMD"] + L.NCMD]
    w, x, y, z = (a[..., X["BQUAT"] + k] for k in range(4))
    roll = np.arctan2(two * (w * x + y * z), one - two * (x * x + y * y))
    pitch = np.arcsin(np.minimum(one, np.maximum(-one, two * (w * y - z * x))))
    yaw = np.arctan2(two * (w * z + x * y), one - two * (y * y + z * z))

    def e2q(r, p, yw):
        cr, sr, cp, sp, cy, sy = np.cos(r / two), np.sin(r / two), np.cos(p / two), np.sin(p / two), np.cos(yw / two), np.sin(yw / two)
        return cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy

    zero = np.zeros_like(yaw)
    out = np.zeros(a.shape[:-1] + (NE,), f)
    # linvel: the command's xy rotated by the base yaw (rotate_by_quat: normalise, matrix, product)
    q = e2q(zero, zero, yaw)
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    qw, qx, qy, qz = (c / n for c in q)
    m0, m1, m2 = one - two * (qy * qy + qz * qz), two * (qx * qy - qw * qz), two * (qx * qz + qw * qy)
    m3, m4, m5 = two * (qx * qy + qw * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qw * qx)
    g0 = m0 * cmd[..., 0] + m1 * cmd[..., 1] + m2 * zero
    g1 = m3 * cmd[..., 0] + m4 * cmd[..., 1] + m5 * zero
    ex, ey = a[..., X["QVEL"]] - g0, a[..., X["QVEL"] + 1] - g1
    out[..., R["LIN"]] = np.sqrt(ex * ex + ey * ey)
    out[..., R["YAW"]] = np.abs(a[..., X["QVEL"] + 5] - cmd[..., 2])
    q1, q2 = e2q(roll, pitch, zero), e2q(cmd[..., 4], cmd[..., 5], zero)
    d = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3]
    out[..., R["TILT"]] = one - d * d
    foh, sh = f(np.float32(foot_origin_height)), f(np.float32(standard_height))
    low = np.minimum(a[..., X["LFZ"]] - foh, a[..., X["RFZ"]] - foh)
    h = a[..., X["BASEZ"]] - low
    target = cmd[..., 3] + sh
    out[..., R["HEIGHT"]] = np.abs(h - target)
    s = np.zeros_like(yaw)
    arm_mag = 0.0
    for j in range(10):
        tj = cmd[..., 6 + j] + f(np.float32(joint_bias[10 + j]))
        dq = a[..., X["ARMQ"] + j] - tj
        s = s + dq * dq
        arm_mag = max(arm_mag, float(np.abs(a[..., X["ARMQ"] + j]).max()), float(np.abs(tj).max()))
    out[..., R["ARM"]] = s
    amax = lambda *v: max(float(np.abs(u).max()) for u in v)
    mag = np.array([amax(a[..., X["QVEL"]], a[..., X["QVEL"] + 1], g0, g1), amax(a[..., X["QVEL"] + 5], cmd[..., 2]), 1.0,
                    amax(a[..., X["BASEZ"]], low, h, target), max(arm_mag, float(s.max()))])
    return out, mag


# ---- part 3: mode, settle scan, statistics ----
def mode_of(cmd) -> int:
    """The KBJ_CMODE of one command: plain comparisons with zero (-0.0 == 0.0)."""
    nz = [float(c) != 0.0 for c in cmd[:3]]
    pose = any(float(c) != 0.0 for c in cmd[3:L.NCMD])
    if not any(nz):
        return M["STAND_BEND"] if pose else M["STAND"]
    if pose or sum(nz) != 1:
        return M["OMNI"]
    return nz.index(True)


def tracking_ref(acc, err, aux, settle_steps):
    """acc [N, 20] float32 (updated IN PLACE), err [T, N, >= 5] float32 error columns (the values to accumulate), aux [T(+1), N, 72].
    Returns (stats [TRK SIZE] float64, mags {slot index: sum |x_i|}, rows [T, N, 3] = mode, settled, since of every row)."""
    T, N = err.shape[:2]
    rows = np.zeros((T, N, 3))
    per_mode = [dict(rows=0, vals=[]) for _ in range(M["COUNT"])]
    changes = episodes = 0
    for n in range(N):
        prev, since, running = acc[n, A["CMD"]:A["CMD"] + L.NCMD].copy(), float(acc[n, A["SINCE"]]), float(acc[n, A["RUNNING"]])
        for t in range(T):
            cmd = aux[t, n, X["CMD"]:X["CMD"] + L.NCMD]
            changed = any(np.float32(cmd[k]) != np.float32(prev[k]) for k in range(L.NCMD))
            if running == 0:
                episodes += 1
                since = 0.0
            elif changed:
                changes += 1
                since = 0.0
            else:
                since = min(since + 1.0, 2.0 ** 24)
            settled = since >= settle_steps
            mode = mode_of(cmd)
            per_mode[mode]["rows"] += 1
            if settled:
                per_mode[mode]["vals"].append([float(v) for v in err[t, n, :NE]])
            rows[t, n] = (mode, float(settled), since)
            prev, running = cmd.copy(), float(aux[t, n, X["DONE"]] == 0)
        acc[n, A["CMD"]:A["CMD"] + L.NCMD], acc[n, A["SINCE"]], acc[n, A["RUNNING"]] = prev, since, running
    st, mags = np.zeros(K["SIZE"], np.float64), {}
    for m, pm in enumerate(per_mode):
        b = m * K["MODE_STRIDE"]
        st[b + K["ROWS"]], st[b + K["SETTLED"]] = pm["rows"], len(pm["vals"])
        for k in range(NE):
            xs = [v[k] for v in pm["vals"]]
            st[b + K["SUM"] + k], mags[b + K["SUM"] + k] = math.fsum(xs), math.fsum(abs(v) for v in xs)
            st[b + K["SUMSQ"] + k] = mags[b + K["SUMSQ"] + k] = math.fsum(v * v for v in xs)
            st[b + K["MAX"] + k] = max(xs, default=0.0)
    st[K["CHANGES"]], st[K["EPISODES"]] = changes, episodes
    return st, mags, rows


def assert_stats_match(got, want, mags, rel=1e-9):
    """Counts and maxima exactly; every double sum within rel * sum |x_i| of the fsum value; every other slot 0."""
    got = np.asarray(got, np.float64)
    for i in range(K["SIZE"]):
        if i in mags:
            assert abs(got[i] - want[i]) <= rel * mags[i], ("sum slot", i, got[i], want[i], mags[i])
        else:
            assert got[i] == want[i], ("exact slot", i, got[i], want[i])


# ---- the synthetic problems ----
def _command(rng, mode):
    """A command of `mode` as UnifiedCommand draws them (train.py:727-749), magnitudes away from zero (and |cmd[0:3]| away from the 1e-3 of the
    rewards' zero-command test), some zeros written as -0.0."""
    c = np.zeros(L.NCMD, np.float32)
    mov = lambda: np.float32(rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 1.0))
    if mode == M["FORWARD"]:
        c[0] = mov()
    elif mode == M["SIDEWAYS"]:
        c[1] = mov()
    elif mode == M["ROTATE"]:
        c[2] = mov()
    elif mode == M["OMNI"]:
        if rng.random() < 0.5:                       # moving with arms (the reference's omni), or two velocities and no pose
            c[0], c[1], c[2] = mov(), mov(), mov()
            c[6:] = rng.uniform(-0.5, 0.5, 10) * (rng.random(10) < 0.5)
            c[6] = np.float32(0.3)
        else:
            c[0], c[2] = mov(), mov()
    elif mode == M["STAND_BEND"]:
        c[3], c[4], c[5] = rng.uniform(-0.25, 0.05), rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25)
        c[6:] = rng.uniform(-0.5, 0.5, 10) * (rng.random(10) < 0.5)
        c[3] = c[3] if c[3] != 0 else np.float32(-0.1)
    zeros = np.flatnonzero(c == 0)
    if zeros.size and rng.random() < 0.3:
        c[rng.choice(zeros)] = np.float32(-0.0)
    return c


class Problems:
    """The chained calls of one shape: `calls[i]` = aux [T + 1, N, 72] float32 of call i. Planted, when there are that many envs and steps:
    env 0 changes its command on row 0 of every call (against the carried one, from the second call on); env 1 never changes its command and
    never ends an episode (an unchanged command across the call boundaries, SINCE growing through them), in the second call with every zero
    of its command written as -0.0 (no change); env 2 has two consecutive DONE rows; the last env ends an episode on the last row of every call."""

    def __init__(self, T, N, seed=None):
        rng = np.random.default_rng(1000 * T + N if seed is None else seed)
        self.T, self.N, self.calls = T, N, []
        cur = np.stack([_command(rng, int(rng.integers(0, M["COUNT"]))) for _ in range(N)])
        for call in range(CALLS):
            aux = np.zeros((T + 1, N, X["SIZE"]), np.float32)
            aux[:T, :, X["QVEL"]:X["QVEL"] + 6] = rng.uniform(-1.5, 1.5, (T, N, 6))
            r, p, yw = rng.uniform(-0.4, 0.4, (T, N)), rng.uniform(-0.4, 0.4, (T, N)), rng.uniform(-np.pi, np.pi, (T, N))
            cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(yw / 2), np.sin(yw / 2)
            aux[:T, :, X["BQUAT"]:X["BQUAT"] + 4] = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                                                             cr * cp * sy - sr * sp * cy], -1)
            aux[:T, :, X["BASEZ"]] = rng.uniform(0.5, 1.0, (T, N))
            aux[:T, :, X["LFZ"]], aux[:T, :, X["RFZ"]] = rng.uniform(0.0, 0.3, (T, N)), rng.uniform(0.0, 0.3, (T, N))
            aux[:T, :, X["ARMQ"]:X["ARMQ"] + 10] = rng.uniform(-1.0, 1.0, (T, N, 10))
            aux[:T, :, X["CTRL"]:X["CTRL"] + L.NU] = rng.uniform(-20, 20, (T, N, L.NU))     # read by kbj_rewards only
            done = np.where(rng.random((T, N)) < 0.1, rng.choice(np.array([-1, 1], np.float32), (T, N)), 0).astype(np.float32)
            done[T - 1, N - 1] = -1
            if N >= 4:
                done[:, 1] = 0
                if T >= 3:
                    done[1, 2], done[2, 2] = -1, 1
            for t in range(T):
                for n in range(N):
                    fixed = N >= 4 and n == 1
                    planted = n == 0 and t == 0
                    if planted or (not fixed and rng.random() < 0.15):
                        new = _command(rng, int(rng.integers(0, M["COUNT"])))
                        while planted and np.array_equal(new, cur[n]):
                            new = _command(rng, int(rng.integers(0, M["COUNT"])))
                        cur[n] = new
                    aux[t, n, X["CMD"]:X["CMD"] + L.NCMD] = cur[n]
            if N >= 4 and call == 1:
                c = aux[:T, 1, X["CMD"]:X["CMD"] + L.NCMD]
                c[c == 0] = np.float32(-0.0)
            aux[:T, :, X["DONE"]] = done
            self.calls.append(aux)


@functools.lru_cache(maxsize=None)
def problems(T, N):
    return Problems(T, N)


def joint_bias():
    from kbot_joystick_amd.spec import constants
    return np.array(constants.JOINT_BIASES, np.float32)


@functools.lru_cache(maxsize=None)
def spread():
    """(S, Mag, per_problem): S[k] = the largest |float32 - float64| of error k over every synthetic problem, Mag[k] = its largest operand
    magnitude there; per_problem[(T, N, call)] = (err64, err32). Computed once, shared by the tests."""
    S, mag, per = np.zeros(NE), np.zeros(NE), {}
    jb = joint_bias()
    for T, N in SHAPES:
        for call, aux in enumerate(problems(T, N).calls):
            e64, m64 = errors(aux[:T], jb, STANDARD_HEIGHT, FOOT_ORIGIN_HEIGHT, np.float64)
            e32, _ = errors(aux[:T], jb, STANDARD_HEIGHT, FOOT_ORIGIN_HEIGHT, np.float32)
            S = np.maximum(S, np.abs(e32.astype(np.float64) - e64).reshape(-1, NE).max(0))
            mag = np.maximum(mag, m64)
            per[(T, N, call)] = (e64, e32)
    return S, mag, per


def error_bounds():
    """The bound of each error column against the float64 reference: max(4 S_k, 8 * 2^-24 * M_k) - 4 x the float32 restatement's own
    distance from float64 (the factor tests/test_gpu_deploy.py grants: device libm and contraction differ from numpy's), and never below
    8 float32 roundings of the largest operand."""
    S, mag, _ = spread()
    return np.maximum(4 * S, 8 * 2.0 ** -24 * mag)


def bounds_for(aux, jb, standard_height, foot_origin_height):
    """(err64, bounds) of other aux rows (a task's own trajectory): the same rule, max(4 S_k, 8 * 2^-24 * M_k), from those rows' own spread
    and operands."""
    e64, mag = errors(aux, jb, standard_height, foot_origin_height, np.float64)
    e32, _ = errors(aux, jb, standard_height, foot_origin_height, np.float32)
    S = np.abs(e32.astype(np.float64) - e64).reshape(-1, NE).max(0)
    return e64, np.maximum(4 * S, 8 * 2.0 ** -24 * mag)
