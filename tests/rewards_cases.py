"""Planted aux rows for the reward stack: deterministic tensors built directly (a seeded default_rng, no env step), in which every branch of
rewards_kernel fires in known rows. tests/test_rewards_ref.py proves the census, the margins and the bounds of these cases on the CPU;
tests/test_gpu_rewards.py runs them through kbj_rewards. Sizes: N in {1, 65, 130} - one thread; a full 64-lane workgroup and one lane; two
and two lanes - and T <= 24."""
import functools

import numpy as np

from kbot_joystick_amd.spec import constants, layout as L
from tests import rewards_ref as RR

X, RC = L.AUX, L.RC
SIZES = (1, 65, 130)
SPARE_WORDS = np.array([0xDEADBEEF, 0x00C0FFEE, 0x3F800001], np.uint32).view(np.float32)     # carry words 5..7: no reader, no writer

# "every branch": the script of one env, row by row. Command kind: W walking (all three velocities), S lateral only (no yaw: the rpy sum of
# feet_orient away from a zero command), Y yaw only, Z zero. L / R: the foot touches. D: the done flag. C: COMDIST's sign (+, -, 0 exactly).
#            t = 0         1         2
#                012345678901234567890123
SCRIPT_KIND = "WWWWWWWWSSSSYYYZZZZWWWWW"
SCRIPT_L    = "100011001111111110111000"
SCRIPT_R    = "111110001001001111111111"
SCRIPT_D    = "0000000000+000-000000000"
SCRIPT_C    = "+-+-+-+-+-+-+-++-+0+-+-+"
# What the script crosses (left / right as written; odd envs run it mirrored):
#   rows 1-3 L in the air under single contact, row 4 L touches down (first, 0.06 s paid), tsingle 0 -> 0.02;
#   rows 6-7 both feet in the air (no_contact, tsingle accumulates), row 8 both touch down (two pay-outs, 0.04 and 0.06 s);
#   row 10 a time-out with R in the air (air time cleared), row 11 R touches down with 0 s (pays -penalty) and base_accel is masked;
#   row 14 R touches down ON a done row (no pay-out, air time cleared), row 15 masked again;
#   rows 15-18 zero command: COMDIST > 0, < 0, > 0 (L lifting: air time runs under a zero command), == 0 (L's touchdown, paid nothing);
#   row 19 the first walking row after a zero command: tsingle was forced to the grace period, so single_contact is 0 until row 21;
#   rows 21-23 L in the air again: the call ends in the middle of a flight phase.
SPLITS = (1, 3, 7, 12, 23)      # a call boundary after 1 row, in L's flight (single contact), with both feet in the air, at T / 2, at T - 1

# The edited grace period is EXACTLY two control steps in float32 (0.02f + 0.02f is exact): after two rows of double support the timer equals
# it bit for bit, in any precision, so `ts < grace` and `ts <= grace` part there - on rows whose decision no rounding can move.
GRACE_2DT = float(np.float32(0.02) + np.float32(0.02))
EDITED = dict(rew_linvel_err=0.35, rew_angvel_err=0.3, rew_rollpitch_err=0.05, rew_rollpitch_err_zero=0.02, rew_height_err=0.05,
              rew_standard_height=0.75, rew_foot_origin_height=0.04, rew_armpos_err=0.2, rew_grace_period=GRACE_2DT, rew_touchdown_penalty=0.2,
              rew_feetorient_err=0.05, rew_comdist_err=0.08, rew_baseaccel_err=3.0, rew_torque_err=2.0)
EDITED_SCALES = (0.3, 0.25, 0.1, 0.4, 0.15, 0.2, -0.3, 0.7, 0.05, 0.2, 0.35, 0.6)


def joint_bias():
    return np.array(constants.JOINT_BIASES, np.float32)


def config(case, n):
    cfg = L.default_config(num_envs=n, batch_size=n, hidden_size=64, rollout_len=8, **case.overrides)
    if case.scales is not None:
        for k, v in enumerate(case.scales):
            cfg.reward_scale[k] = v
    return cfg


# ---- pieces ----
def _command(rng, kind):
    c = np.zeros(L.NCMD, np.float32)
    mov = lambda lo, hi: rng.choice([-1.0, 1.0]) * rng.uniform(lo, hi)
    if kind == "W":
        c[0], c[1], c[2] = mov(0.1, 1.2), mov(0.1, 0.5), mov(0.1, 1.0)
    elif kind == "S":
        c[1] = mov(0.1, 0.5)
    elif kind == "Y":
        c[2] = mov(0.1, 1.0)
    elif rng.random() < 0.5:
        c[:3] = rng.uniform(-3e-4, 3e-4, 3)              # a "zero" command that is not zero: |cmd[0:3]| <= 5.2e-4
    c[3], c[4], c[5] = rng.uniform(-0.25, 0.05), rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25)
    c[6:] = rng.uniform(-0.5, 0.5, 10) * (rng.random(10) < 0.5)
    return c


def _straight_feet(yaw, rng, spread):
    """[..., 2, 4]: the straight foot of train.py:420-440 (-+pi/2, 0, base yaw - pi), each angle off by N(0, spread)."""
    n = lambda: rng.normal(0, spread, yaw.shape) if spread else 0.0
    return np.stack([RR.euler_to_quat(-np.pi / 2 + n(), n() + 0 * yaw, yaw - np.pi + n()), RR.euler_to_quat(np.pi / 2 + n(), n() + 0 * yaw, yaw - np.pi + n())], -2)


def _rows(rng, cmd, con, done, cd_sign, tilt=0.3):
    """Plausible rows around planted commands [T, N, 16], contacts [T, N, 2], done [T, N] and COMDIST signs [T, N] (+1, -1, 0)."""
    T, N = done.shape
    jb = joint_bias()
    aux = np.zeros((T, N, X["SIZE"]), np.float32)
    aux[..., X["QVEL"]:X["QVEL"] + 6] = rng.uniform(-1, 1, (T, N, 6))
    roll, pitch, yaw = rng.uniform(-tilt, tilt, (T, N)), rng.uniform(-tilt, tilt, (T, N)), rng.uniform(-np.pi, np.pi, (T, N))
    aux[..., X["BQUAT"]:X["BQUAT"] + 4] = RR.euler_to_quat(roll, pitch, yaw)
    aux[..., X["BASEZ"]] = rng.uniform(0.7, 0.95, (T, N))
    aux[..., X["LFZ"]], aux[..., X["RFZ"]] = rng.uniform(0.03, 0.2, (T, N)), rng.uniform(0.03, 0.2, (T, N))
    feet = _straight_feet(yaw, rng, 0.08)
    aux[..., X["LFQUAT"]:X["LFQUAT"] + 4], aux[..., X["RFQUAT"]:X["RFQUAT"] + 4] = feet[..., 0, :], feet[..., 1, :]
    aux[..., X["ARMQ"]:X["ARMQ"] + 10] = cmd[..., 6:16] + jb[10:20] + rng.uniform(-0.15, 0.15, (T, N, 10))
    aux[..., X["CTRL"]:X["CTRL"] + L.NU] = rng.uniform(-20, 20, (T, N, L.NU))
    aux[..., X["TOUCH"]:X["TOUCH"] + 2] = np.where(con, rng.uniform(0.5, 60, (T, N, 2)), np.where(rng.random((T, N, 2)) < 0.5, 0.0, rng.uniform(0, 0.05, (T, N, 2))))
    aux[..., X["COMDIST"]] = np.where(cd_sign > 0, rng.uniform(0.002, 0.12, (T, N)), np.where(cd_sign < 0, -1.0, 0.0))
    aux[..., X["CMD"]:X["CMD"] + L.NCMD] = cmd
    aux[..., X["DONE"]] = done
    return aux


def _carry(rng, n, P):
    """A carry no reset leaves: a running timer, air times on feet that were off the ground, the spare words marked."""
    rc = RR.initial_carry(n)
    pcon = rng.random((n, 2)) < 0.5
    dt = np.float32(P.ctrl_dt)
    rc[:, RC["TSINGLE"]] = rng.integers(0, 4, n).astype(np.float32) * dt
    rc[:, RC["AIRTIME"]:RC["AIRTIME"] + 2] = np.where(pcon, 0, rng.integers(1, 6, (n, 2)).astype(np.float32) * dt)
    rc[:, RC["CONTACT"]:RC["CONTACT"] + 2] = pcon
    rc[:, RC["CONTACT"] + 2:] = SPARE_WORDS
    return rc


class Case:
    def __init__(self, name, T, overrides=None, scales=None, own_carry=()):
        self.name, self.T, self.overrides, self.scales, self.own_carry = name, T, overrides or {}, scales, own_carry

    @functools.lru_cache(maxsize=None)
    def problem(self, n):
        """(aux [T, N, 72] float32, carry [N, 8] float32), read-only."""
        rng = np.random.default_rng([sum(map(ord, self.name)), n])
        aux = getattr(self, "_" + self.name)(rng, n)
        rc = _carry(rng, n, RR.Params(config(self, n))) if n in self.own_carry else RR.initial_carry(n)
        aux.setflags(write=False); rc.setflags(write=False)
        return aux, rc

    @functools.lru_cache(maxsize=None)
    def reference(self, n):
        aux, rc = self.problem(n)
        return RR.scan(aux, RR.Params(config(self, n)), joint_bias(), rc)

    # ---- the five cases ----
    def _every_branch(self, rng, n):
        T = self.T
        assert all(len(s) == T for s in (SCRIPT_KIND, SCRIPT_L, SCRIPT_R, SCRIPT_D, SCRIPT_C))
        cmd, con = np.zeros((T, n, L.NCMD), np.float32), np.zeros((T, n, 2), bool)
        for e in range(n):
            for t in range(T):
                if t == 0 or SCRIPT_KIND[t] != SCRIPT_KIND[t - 1]:
                    cur = _command(rng, SCRIPT_KIND[t])
                cmd[t, e] = cur
            lr = (SCRIPT_L, SCRIPT_R) if e % 2 == 0 else (SCRIPT_R, SCRIPT_L)
            con[:, e, 0], con[:, e, 1] = [c == "1" for c in lr[0]], [c == "1" for c in lr[1]]
        done = np.tile(np.array([{"0": 0, "+": 1, "-": -1}[c] for c in SCRIPT_D], np.float32)[:, None], (1, n))
        cd = np.tile(np.array([{"+": 1, "-": -1, "0": 0}[c] for c in SCRIPT_C], np.float32)[:, None], (1, n))
        return _rows(rng, cmd, con, done, cd)

    def _grace_edge(self, rng, n):
        T = self.T
        cmd = np.zeros((T, n, L.NCMD), np.float32)
        for e in range(n):
            w = _command(rng, "W")
            cmd[:, e] = w
            if e % 2 == 0:
                cmd[8:10, e] = _command(rng, "Z")            # forces the timer to the grace period in the middle of the call
        u = rng.random((T, n))
        con = np.stack([u < 0.85, (u < 0.75) | (u >= 0.85) & (u < 0.95)], -1)     # 75 % double, 10 % L only, 10 % R only, 5 % none
        return _rows(rng, cmd, con, np.zeros((T, n), np.float32), np.ones((T, n)))

    def _orientation(self, rng, n):
        T = self.T
        kinds = rng.choice(list("WSYZ"), (T, n))
        cmd = np.stack([[_command(rng, k) for k in row] for row in kinds]).astype(np.float32)
        aux = _rows(rng, cmd, np.ones((T, n, 2), bool), np.zeros((T, n), np.float32), np.where(rng.random((T, n)) < 0.5, 1.0, -1.0))

        def sphere(shape):                                   # uniform on the sphere, away from the pitch singularity
            q = rng.normal(size=shape + (4,))
            q /= np.linalg.norm(q, axis=-1, keepdims=True)
            while True:
                q32 = q.astype(np.float32).astype(np.float64)
                bad = np.abs(2 * (q32[..., 0] * q32[..., 2] - q32[..., 3] * q32[..., 1])) > 0.99
                if not bad.any():
                    return q
                r = rng.normal(size=(int(bad.sum()), 4))
                q[bad] = r / np.linalg.norm(r, axis=-1, keepdims=True)

        bq = sphere((T, n))
        aux[..., X["BQUAT"]:X["BQUAT"] + 4] = bq
        roll, pitch, yaw, _ = RR.quat_to_euler(bq)
        feet = _straight_feet(yaw, rng, 0.08)                # odd rows: near the straight foot of THIS base yaw; even rows: anywhere
        feet[0::2] = sphere((len(range(0, T, 2)), n, 2))
        aux[..., X["LFQUAT"]:X["LFQUAT"] + 4], aux[..., X["RFQUAT"]:X["RFQUAT"] + 4] = feet[..., 0, :], feet[..., 1, :]
        aux[1::2, :, X["CMD"] + 4] = (roll + rng.normal(0, 0.05, (T, n)))[1::2]      # a commanded tilt near the base's own, however large
        aux[1::2, :, X["CMD"] + 5] = (pitch + rng.normal(0, 0.05, (T, n)))[1::2]
        # the clamp: quaternions 0.05 % too long at pitch = +-90 degrees, 2 (w y - z x) = +-1.001
        h = 1.0005 * np.sqrt(0.5)
        for t, e, col, sgn in ((3, 0, "BQUAT", 1), (5, 64, "BQUAT", -1), (7, 129, "BQUAT", 1), (9, 0, "LFQUAT", -1), (11, 64, "RFQUAT", 1)):
            if e < n:
                aux[t, e, X[col]:X[col] + 4] = (h, 0, sgn * h, 0)
        return aux

    def _edited_table(self, rng, n):
        T = self.T
        cmd = np.zeros((T, n, L.NCMD), np.float32)
        for e in range(n):
            for t in range(T):
                if t == 0 or rng.random() < 0.25:
                    cur = _command(rng, rng.choice(list("WSYZ")))
                cmd[t, e] = cur
        con = np.zeros((T, n, 2), bool)
        state = rng.random((n, 2)) < 0.7
        for t in range(T):
            state = np.where(rng.random((n, 2)) < 0.3, ~state, state)
            con[t] = state
        done = np.where(rng.random((T, n)) < 0.08, rng.choice([-1.0, 1.0], (T, n)), 0.0).astype(np.float32)
        return _rows(rng, cmd, con, done, np.where(rng.random((T, n)) < 0.6, 1.0, -1.0))

    def _small_errors(self, rng, n):
        """Every tracking error within 1e-3 of zero, every torque within 1e-2: all the exp terms within a few hundred ulp of 1."""
        T = self.T
        jb = joint_bias()
        cmd = np.zeros((T, n, L.NCMD), np.float32)
        for e in range(n):
            cmd[:, e] = _command(rng, "WSYZ"[e % 4])
        con = np.ones((T, n, 2), bool)
        con[(np.arange(T) % 4 == 1)[:, None] & (np.arange(n) % 2 == 0)[None, :], 0] = False
        aux = _rows(rng, cmd, con, np.zeros((T, n), np.float32), np.ones((T, n)))
        c = cmd.astype(np.float64)
        yaw = np.tile(rng.uniform(-np.pi, np.pi, n), (T, 1))
        bq = RR.euler_to_quat(c[..., 4] + rng.uniform(-2e-4, 2e-4, (T, n)), c[..., 5] + rng.uniform(-2e-4, 2e-4, (T, n)), yaw).astype(np.float32)
        aux[..., X["BQUAT"]:X["BQUAT"] + 4] = bq
        _, _, yaw32, _ = RR.quat_to_euler(bq.astype(np.float64))                     # the yaw the rounded quaternion really has
        qv = rng.uniform(-3e-5, 3e-5, (T, n, 6))                                     # steady: base_accel's sum stays below 1e-3
        qv[..., 0] += np.cos(yaw32) * c[..., 0] - np.sin(yaw32) * c[..., 1] + rng.uniform(-5e-4, 5e-4, (T, n))
        qv[..., 1] += np.sin(yaw32) * c[..., 0] + np.cos(yaw32) * c[..., 1] + rng.uniform(-5e-4, 5e-4, (T, n))
        qv[..., 5] += c[..., 2] + rng.uniform(-8e-4, 8e-4, (T, n))
        qv[..., 2:5] += np.tile(rng.uniform(-0.3, 0.3, (1, n, 3)), (T, 1, 1))
        aux[..., X["QVEL"]:X["QVEL"] + 6] = qv
        lfz = rng.uniform(0.06, 0.1, (T, n))
        aux[..., X["LFZ"]], aux[..., X["RFZ"]] = lfz, lfz + rng.uniform(0, 0.05, (T, n))
        aux[..., X["BASEZ"]] = lfz.astype(np.float32) - np.float32(0.06) + c[..., 3] + np.float32(0.80) + rng.uniform(-8e-4, 8e-4, (T, n))
        arm = c[..., 6:16] + jb[10:20] + rng.uniform(-8e-3, 8e-3, (T, n, 10))
        arm[..., 3] = c[..., 9] + jb[13]                                             # a joint that sits at its target
        aux[..., X["ARMQ"]:X["ARMQ"] + 10] = arm
        feet = _straight_feet(yaw32, rng, 3e-3)
        aux[..., X["LFQUAT"]:X["LFQUAT"] + 4], aux[..., X["RFQUAT"]:X["RFQUAT"] + 4] = feet[..., 0, :], feet[..., 1, :]
        aux[..., X["CTRL"]:X["CTRL"] + L.NU] = rng.uniform(-1e-2, 1e-2, (T, n, L.NU))
        aux[..., X["COMDIST"]] = rng.uniform(0, 1e-3, (T, n))
        return aux


CASES = (Case("every_branch", 24, own_carry=(65,)), Case("grace_edge", 24, dict(rew_grace_period=0.05)), Case("orientation", 12),
         Case("edited_table", 16, EDITED, EDITED_SCALES, own_carry=(1, 65, 130)), Case("small_errors", 12))
BY_NAME = {c.name: c for c in CASES}


# ---- the rollout rows of the two older reward tests (what the mutation table's "old criterion" column and their added comparison run on) ----
OLD_EDITED = dict(rew_linvel_err=0.35, rew_rollpitch_err=0.05, rew_standard_height=0.75, rew_grace_period=0.1, rew_touchdown_penalty=0.2, rew_torque_err=2.0)
OLD_EDITED_SCALES = (0.3, 0.0, 0.1, 0.4, 0.0, 0.2, 0.3, 0.7, 0.05, 0.2, 0.0, 0.6)


@functools.lru_cache(maxsize=None)
def rollout(which):
    """(model, cfg, aux [T, N, 72]) of tests/test_gpu_host.py::test_edited_reward_table_matches_oracle ("edited": N = 64, T = 12) or of
    tests/test_gpu_env.py::test_free_running_rollout_statistics ("free": N = 256, T = 60): the fp32 oracle stepped with their seeds and actions."""
    from kbot_joystick_amd.spec import compiler
    from oracle import oracle as O
    from tests import helpers as H
    model = compiler.load_model("kbot-headless")
    if which == "edited":
        N, T, seed, rng, amp = 64, 12, 2, np.random.default_rng(3), 0.5
        cfg = L.default_config(num_envs=N, batch_size=N, **OLD_EDITED)
        for i, s in enumerate(OLD_EDITED_SCALES):
            cfg.reward_scale[i] = s
    else:
        N, T, seed, rng, amp = 256, 60, 3, np.random.default_rng(1), 0.1
        cfg = L.default_config(num_envs=N, batch_size=N)
    o = O.Oracle(model, cfg, seed=seed, precision="f32")
    aux = np.zeros((T + 1, N, X["SIZE"]), np.float32)
    _, _, aux[0] = o.reset_all()
    for t in range(T):
        _, _, aux[t + 1] = o.step(H.random_actions(model, rng, N, amp), aux[t])
    aux = aux[:T].copy()
    aux.setflags(write=False)
    return model, cfg, aux
