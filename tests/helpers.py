"""Shared helpers for the parity tests: env side first, the actor-critic / PPO side (synthetic minibatch problems against oracle/nn.py) below."""
import ctypes as C
import os
import subprocess

import numpy as np

from kbot_joystick_amd.spec.layout import RNG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Parity tolerances for ONE control step (5 substeps) started from the identical fp32 state, MEASURED (profiles/parity_r02.json,
# tools/parity_quantiles.py: 8192 envs x 12 teacher-forced steps, errors against the fp64 oracle):
#              median     p99      p99.9    max
#   HIP  qpos  1.8e-7   7.8e-7   1.4e-6   4.2e-2      oracle fp32  qpos  1.8e-7   8.6e-7   1.6e-6   4.2e-2
#   HIP  qvel  6.6e-7   3.8e-6   7.5e-6   5.4e-1      oracle fp32  qvel  7.2e-7   4.3e-6   8.3e-6   3.3e-1
#   HIP  qacc  2.6e-6   1.7e-5   3.9e-5   1.7e+0      oracle fp32  qacc  2.9e-6   2.0e-5   4.7e-5   4.6e-1
# i.e. the kernel is as close to fp64 as the oracle's own fp32 instantiation, at every quantile. The table below is 2x the oracle's
# own fp32 spread for (median, p99, p99.9); the tests that have the fp64 oracle at hand (check_against_oracle_spread) compare with
# the spread measured in the same run instead of with these constants. The extreme value is set by a handful of env-steps that sit
# on a discrete switch of the solver (contact on/off, friction row saturating, Newton iteration cap: 0.02 % of env-steps, the same
# share in the oracle's fp32-vs-fp64 comparison) and is bounded relative to the oracle's own extreme value.
TOL = dict(qpos=(4e-7, 2e-6, 4e-6, 0.1), qvel=(1.5e-6, 1e-5, 2e-5, 1.0), qacc=(6e-6, 4e-5, 1e-4, 4.0))   # (median, p99, p99.9, max)


def emu_lib(solver: str = "reg", sanitize: bool = False) -> C.CDLL:
    """Host emulation build of the kernel body (tests/emu) — test infrastructure. solver = "reg": the product kernel's register-resident
    Newton solver, its wave primitives (DPP broadcasts, butterflies, lane swaps) emulated lane by lane (kbj_wave.h); "lds": the LDS
    formulation that `make ldssolver` builds for the GPU A/B test. sanitize: -fsanitize=address,undefined (load it in a child process
    with libasan preloaded, tests/test_sanitize.py)."""
    name = "libkbj_emu" + ("" if solver == "reg" else "_lds") + ("_asan" if sanitize else "") + ".so"
    out = os.path.join(ROOT, "tests", "emu", "_build", name)
    src = os.path.join(ROOT, "tests", "emu", "kbj_env_emu.cpp")
    deps = [src] + [os.path.join(ROOT, "kbot-joystick_amd", "csrc", f) for f in ("kbj_env_core.h", "kbj_env_phys.h", "kbj_env_task.h", "kbj_wave.h")]
    deps.append(os.path.join(ROOT, "include", "kbj_model.h"))
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
        if solver == "lds":
            flags.append("-DKBJ_ARROW_LDS")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                               "-shared", "-o", out, src])
    return C.CDLL(out) if not sanitize else out


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def state_errors(es_ref: np.ndarray, es_got: np.ndarray):
    """Per-env error measures between two [N][ES] state arrays."""
    d = np.abs(es_ref.astype(np.float64) - es_got.astype(np.float64))
    return dict(qpos=d[:, 0:27].max(1),
                qvel=d[:, 28:54].max(1) / (1 + np.abs(es_ref[:, 28:54]).max(1)),
                qacc=d[:, 54:80].max(1) / (1 + np.abs(es_ref[:, 54:80]).max(1)))


def check_error_distribution(errs: dict, tol=TOL, label=""):
    for k, (med, p99, p999, mx) in tol.items():
        v = np.concatenate(errs[k])
        assert np.median(v) <= med, f"{label}{k}: median {np.median(v):.3e} > {med}"
        assert np.quantile(v, 0.99) <= p99, f"{label}{k}: p99 {np.quantile(v, 0.99):.3e} > {p99}"
        if v.size >= 20000:     # a 99.9th percentile needs samples
            assert np.quantile(v, 0.999) <= p999, f"{label}{k}: p99.9 {np.quantile(v, 0.999):.3e} > {p999}"
        assert v.max() <= mx, f"{label}{k}: max {v.max():.3e} > {mx}"


def check_against_oracle_spread(err_hip: dict, err_o32: dict, switch: np.ndarray, label=""):
    """HIP-vs-fp64 error distribution against the oracle's own fp32-vs-fp64 distribution measured on the SAME env-steps:
      * median, p99, p99.9 at most 2x the oracle's (floored at a few fp32 roundings of the quantity);
      * no heavier tail: the count of env-steps beyond 2x the oracle's p99.9 is at most 1.5x the oracle's own count (+5);
      * the extreme value inside the absolute bound of the tolerance table (a single env-step on a discrete switch sets it, in
        the oracle's fp32-vs-fp64 comparison just the same: the ratio of two such extremes is not a stable statistic);
      * beyond 2x the oracle's p99.9, at most 8 env-steps that the oracle does not itself flag as sitting on a discrete switch of
        the solver (`switch`: active contacts / force-carrying rows / iteration counts differ between two evaluations that differ
        only by rounding, or the iteration cap bites) - measured: 2-3 of 98k, the kernel's own rounding flips a switch there."""
    floor = dict(qpos=2e-7, qvel=1e-6, qacc=4e-6)
    sw = np.concatenate(switch)
    for k in ("qpos", "qvel", "qacc"):
        h, o = np.concatenate(err_hip[k]), np.concatenate(err_o32[k])
        for name, q in (("median", 0.5), ("p99", 0.99), ("p99.9", 0.999)):
            hq, oq = np.quantile(h, q), np.quantile(o, q)
            assert hq <= 2 * max(oq, floor[k]), f"{label}{k} {name}: HIP {hq:.3e} vs oracle fp32 {oq:.3e}"
        thr = 2 * np.quantile(o, 0.999)
        nh, no = int((h > thr).sum()), int((o > thr).sum())
        assert nh <= 1.5 * no + 5, f"{label}{k}: {nh} env-steps beyond {thr:.2e}, the oracle's fp32 run has {no}"
        assert h.max() <= TOL[k][3], f"{label}{k}: max {h.max():.3e} (oracle fp32 max {o.max():.3e})"
        unexplained = int(((h > thr) & ~sw).sum())
        assert unexplained <= 8, f"{label}{k}: {unexplained} outliers beyond {thr:.2e} on env-steps without a discrete solver switch"


def random_actions(model, rng, n, scale=0.3):
    return (np.tile(np.array(model.joint_bias, np.float32), (n, 1)) + rng.normal(size=(n, 20)).astype(np.float32) * scale)


# ---------------------------------------------------------------------------------------------------------------------
# episode ends: every termination cause, the terminal record and the in-step reset, against the oracle
# (GPU: tests/test_gpu_env.py; the host emulation of the kernel body: tests/test_emu_env.py; the oracle halves alone, which keep
# the cases alive: tests/test_oracle_task.py)
# ---------------------------------------------------------------------------------------------------------------------
# Teacher-forced cases (seed 11, random_actions scale 0.3 from default_rng(0)). `counts`: what the fp32 oracle gives, measured on the
# CPU and pinned there (tests/test_oracle_task.py), `max_episode` = the most episodes one env has finished (the in-step reset then draws
# from episode counter max_episode + 1's slots); `floors`: half of the counts, the liveness the GPU test asserts. The threshold
# config ends episodes while the robot is still in ordinary, contact-stable states (so a normal step's tolerances hold); the default
# config run long enough to fall puts contact-rich states into the terminal records.
EPISODE_END_CASES = {
    "episode ends": dict(N=256, steps=24, cfg=dict(unhealthy_z=0.655, max_tilt_rad=0.12, max_episode_steps=7),
                         counts=dict(height=960, tilt_only=52, timeout=100, fail_on_timeout=175), max_episode=7,
                         floors=dict(height=480, tilt_only=26, timeout=50, fail_on_timeout=87)),
    "falls": dict(N=256, steps=60, cfg=dict(),
                  counts=dict(height=55, tilt_only=175, timeout=0, fail_on_timeout=0), max_episode=2,
                  floors=dict(height=27, tilt_only=87, timeout=0, fail_on_timeout=0)),
}
# terminations the fp32 oracle gives in the default-config cases of test_teacher_forced_steps_match_oracle: (N, steps, command) -> count
TEACHER_FORCED_TERMINATIONS = {(128, 30, "sampler"): 5, (8192, 12, "sampler"): 0, (8192, 6, "fixed"): 0, (256, 20, "sampler on jax.random keys"): 0}

# column groups of the completed aux_t record: name -> (first column, width, floor). The floor is a few fp32 roundings of the
# quantity: velocities and positions as in check_against_oracle_spread (qvel 1e-6, qpos 2e-7); unit quaternion components and heights
# below 1 m like positions; a PD torque is kp (~100) times a position error plus kd times a velocity error, values up to ~40 N m whose
# one rounding is 4e-6: 2e-5.
AUX_RECORD_GROUPS = dict(QVEL=(0, 6, 1e-6), BQUAT=(6, 4, 2e-7), HEIGHTS=(10, 3, 2e-7), FOOTQUAT=(13, 8, 2e-7), ARMQ=(21, 10, 2e-7), CTRL=(31, 20, 2e-5))


class Step:
    """What one control step leaves behind, as host arrays: parameter / state rows, the completed aux_t row, the next rows."""
    def __init__(self, ep, es, aux_t, actor, critic, aux):
        self.ep, self.es, self.aux_t, self.actor, self.critic, self.aux = ep, es, aux_t, actor, critic, aux


def record_height(aux_t):
    """The height termination's operand (kbj_env_task.h task_step: xpos[base].z - fminf(xpos[lfoot].z, xpos[rfoot].z)) from a record, in fp64."""
    from kbot_joystick_amd.spec import layout as L
    x = aux_t.astype(np.float64)
    return x[:, L.AUX["BASEZ"]] - np.minimum(x[:, L.AUX["LFZ"]], x[:, L.AUX["RFZ"]])


def record_tilt_zz(aux_t):
    """The tilt termination's expression (kbj_env_task.h task_step: zz = 1 - 2 (qx qx + qy qy), failing below cos(max_tilt_rad)) on a record's
    base quaternion, in fp64. The record holds the quaternion of the last substep's kinematics, the kernel tests the integrated one: a
    margin taken here is that of the record, one substep (4 ms) before the state the flag was decided on (zz moves by up to 2e-3 in that
    substep in the "episode ends" case, 1.7e-2 in "falls"; on the integrated state the smallest fp64 margins are 1.1e-6 and 9.3e-5, measured
    with a second oracle whose thresholds are off). A flag that flips on the tilt threshold is therefore excused only where the record
    happens to sit on the threshold too: the exemption is in practice the height test's."""
    from kbot_joystick_amd.spec import layout as L
    q = aux_t[:, L.AUX["BQUAT"]:L.AUX["BQUAT"] + 4].astype(np.float64)
    return 1 - 2 * (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])


class EpisodeEndAudit:
    """Accumulates, over the steps of a teacher-forced run, everything about the END of an episode that an implementation of the control
    step (`got`: the HIP kernel, or its host emulation) must share with the oracle; `got` = None audits the oracle halves alone.

    add() per step, from the identical start state `es0`:
      * DONE against the fp32 oracle's, sign included. A disagreement is kept for finish(), which excuses it only if it is a failure flag
        (-1 against the time-out / running value that is due) on an env-step whose fp64 margin to the height or tilt threshold is below
        4x the largest fp32-vs-fp64 oracle error of that quantity in this run, and at most `max_exempt` of them;
      * the per-cause counts, from the oracle's flags;
      * rows that both sides finish: the new episode's parameters and state with the fields and bounds of test_reset_matches_oracle (exact,
        base quaternion 3e-7: device libm against glibc), the cleared warm start, the re-seeded lagged projected gravity, and the new
        episode's first actor / critic / aux rows with that test's bounds;
      * the completed aux_t row by column group, error against the fp64 oracle beside the fp32 oracle's own on the same env-steps,
        terminal and running rows apart.
    finish() asserts what needs the whole run and returns the measured figures."""

    def __init__(self, cfg, max_exempt=2, label=""):
        self.max_steps, self.max_exempt, self.label = int(cfg.max_episode_steps), max_exempt, label
        self.uz = float(np.float32(cfg.unhealthy_z))                       # the threshold as the fp64 oracle reads it: the fp32 field, widened
        self.cos_tilt = float(np.cos(np.float64(np.float32(cfg.max_tilt_rad))))
        self.counts = dict(height=0, tilt_only=0, timeout=0, fail_on_timeout=0)
        self.oracle_flips, self.max_episode, self.t = 0, 0, 0
        self.err_height, self.err_zz = 0.0, 0.0                            # largest fp32-vs-fp64 oracle error of the two operands
        self.margin_height, self.margin_zz = np.inf, np.inf                # smallest fp64 distance to the thresholds
        self.disagree = []                                                 # (t, env, got, oracle, due, margin_height, margin_zz)
        self.rec_got = {g: [] for g in AUX_RECORD_GROUPS}
        self.rec_o32 = {g: [] for g in AUX_RECORD_GROUPS}
        self.terminal, self.switch = [], []
        self.reset_rows = 0
        self.reset_err = dict(quat=0.0, pglag=0.0, actor=0.0, critic=0.0, aux=0.0)
        self.o32_reset_err = dict(state=0.0, quat=0.0, pglag=0.0, actor=0.0, critic=0.0, aux=0.0)

    def add(self, es0, o32: Step, o64: Step, got: Step = None, switch=None):
        """One step. Returns the rows whose DONE is the oracle's (all rows where `got` is None)."""
        from kbot_joystick_amd.spec import layout as L
        t, self.t = self.t, self.t + 1
        d32, d64 = o32.aux_t[:, L.AUX["DONE"]], o64.aux_t[:, L.AUX["DONE"]]
        due = es0[:, L.ES["TIME"]] + 1 >= self.max_steps
        h64, z64 = self._collect_oracle(o32, o64, d32, d64, due)
        if got is None:
            return np.ones_like(due)
        dg = got.aux_t[:, L.AUX["DONE"]]
        agree = dg == d32
        for i in np.nonzero(~agree)[0]:
            self.disagree.append((t, int(i), float(dg[i]), float(d32[i]), bool(due[i]), float(abs(h64[i] - self.uz)), float(abs(z64[i] - self.cos_tilt))))
        both = (d32 != 0) & (d64 != 0) & agree
        if both.any():
            self._assert_reset_rows(es0, o32, got, both, (self.label, t))
        self._collect_record(o32, o64, got, agree, (d32 != 0), np.zeros_like(due) if switch is None else switch)
        return agree

    def _collect_oracle(self, o32, o64, d32, d64, due):
        """The oracle halves of a step: per-cause counts from the fp32 oracle's flags, fp32 / fp64 flips, the operands' errors and margins,
        and the two precisions' disagreement on the rows both reset (the yardstick of the post-reset bounds). Returns the fp64 operands."""
        from kbot_joystick_amd.spec import layout as L
        h32, h64, z32, z64 = record_height(o32.aux_t), record_height(o64.aux_t), record_tilt_zz(o32.aux_t), record_tilt_zz(o64.aux_t)
        self.oracle_flips += int((d32 != d64).sum())
        self.err_height, self.err_zz = max(self.err_height, float(np.abs(h32 - h64).max())), max(self.err_zz, float(np.abs(z32 - z64).max()))
        self.margin_height = min(self.margin_height, float(np.abs(h64 - self.uz).min()))
        self.margin_zz = min(self.margin_zz, float(np.abs(z64 - self.cos_tilt).min()))
        fail, low = d32 == -1, h64 < self.uz
        self.counts["height"] += int((fail & low).sum())
        self.counts["tilt_only"] += int((fail & ~low).sum())
        self.counts["timeout"] += int((d32 == 1).sum())
        self.counts["fail_on_timeout"] += int((fail & due).sum())
        assert np.isin(d32, (-1.0, 0.0, 1.0)).all() and not (d32[~due] == 1).any()
        self.max_episode = max(self.max_episode, int(o32.es[:, L.ES["EPISODE"]].view(np.uint32).max()) - 1)      # env_reset_all starts at counter 1
        both = (d32 != 0) & (d64 != 0)
        if both.any():
            e = self.o32_reset_err
            cols = np.r_[0:3, 7:27, 28:125, 128:130]
            bits32, bits64 = o32.es[both][:, cols].view(np.uint32).astype(np.int64), o64.es[both][:, cols].view(np.uint32).astype(np.int64)
            e["state"] = max(e["state"], float(np.abs(bits32 - bits64).max()), float(np.abs(o32.ep[both] - o64.ep[both]).max()))
            for k, v in self._reset_errors(o64, o32, both).items():
                e[k] = max(e[k], v)
        return h64, z64

    def _assert_reset_rows(self, es0, o32, got, both, lab):
        """Rows that the oracle and `got` both finish: the new episode, as test_reset_matches_oracle holds kbj_env_reset_all at episode 0."""
        from kbot_joystick_amd.spec import layout as L
        self.reset_rows += int(both.sum())
        o, g = o32.es[both], got.es[both]
        assert np.array_equal(o32.ep[both], got.ep[both]), lab                                   # the new episode's randomised parameters
        assert np.array_equal(o[:, 0:3], g[:, 0:3]) and np.array_equal(o[:, 7:27], g[:, 7:27]), lab
        assert np.abs(o[:, 28:54] - g[:, 28:54]).max() == 0, lab                                 # qvel
        assert (g[:, 54:80] == 0).all() and (o[:, 54:80] == 0).all(), lab                        # the warm start, cleared
        assert np.array_equal(o[:, 80:125], g[:, 80:125]), lab                                   # ACT_PREV, command, push block, time
        assert np.array_equal(o[:, 128:130].view(np.uint32), g[:, 128:130].view(np.uint32)), lab   # episode / step counters ...
        assert np.array_equal(g[:, 128:130].view(np.uint32), es0[both, 128:130].view(np.uint32) + 1) and (g[:, L.ES["TIME"]] == 0).all(), lab   # ... each + 1, time restarted
        e = self.reset_err
        for k, v in self._reset_errors(o32, got, both).items():
            e[k] = max(e[k], v)
        assert e["quat"] < 3e-7, (lab, e)                      # cosf / sinf(yaw / 2): device libm vs glibc, 1-2 ulp
        # The lagged gravity is re-seeded with the projected gravity of the new episode's forward kinematics: a unit vector turned by the
        # new base quaternion. The two oracle precisions give it bit-identically (pinned in tests/test_oracle_task.py), so no oracle
        # spread sets this bound. It is the existing bound of the host emulation's reset (tests/test_emu_env.py: the kinematics compose
        # the rotations in another order), and what the quaternion bound above implies: a rotation is quadratic in the quaternion,
        # 2 x 3e-7 per component, plus the roundings of the products.
        assert e["pglag"] < 1e-6, (lab, e)
        assert e["actor"] < 1e-4 and e["critic"] < 1e-3 and e["aux"] < 1e-4, (lab, e)

    def _collect_record(self, o32, o64, got, agree, terminal, switch):
        """The completed aux_t row by column group: `got`'s and the fp32 oracle's error against the fp64 oracle on the same env-steps."""
        ref = o64.aux_t.astype(np.float64)
        for name, (c0, w, _) in AUX_RECORD_GROUPS.items():
            self.rec_got[name].append(np.abs(got.aux_t[agree, c0:c0 + w] - ref[agree, c0:c0 + w]).max(1))
            self.rec_o32[name].append(np.abs(o32.aux_t[agree, c0:c0 + w] - ref[agree, c0:c0 + w]).max(1))
        self.terminal.append(terminal[agree])
        self.switch.append(switch[agree])

    @staticmethod
    def _reset_errors(ref: Step, got: Step, rows):
        from kbot_joystick_amd.spec import layout as L
        c0 = ref.critic[rows]
        return dict(quat=float(np.abs(ref.es[rows, 3:7] - got.es[rows, 3:7]).max()),
                    pglag=float(np.abs(ref.es[rows, L.ES["PGLAG"]:L.ES["PGLAG"] + 3] - got.es[rows, L.ES["PGLAG"]:L.ES["PGLAG"] + 3]).max()),
                    actor=float(np.abs(ref.actor[rows] - got.actor[rows]).max()),
                    critic=float((np.abs(c0 - got.critic[rows]) / (1 + np.abs(c0))).max()),
                    aux=float(np.abs(ref.aux[rows] - got.aux[rows]).max()))

    def finish(self, floors=None, verbose=True):
        lab = self.label
        for name, floor in (floors or {}).items():                # liveness: every cause occurs, from the oracle's flags
            assert self.counts[name] >= floor, f"{lab}{name}: {self.counts[name]} env-steps, the case needs {floor}"
        assert self.oracle_flips == 0, f"{lab}the fp32 and fp64 oracle disagree on {self.oracle_flips} DONE flags: the case sits on a threshold"
        bound_h, bound_z = 4 * self.err_height, 4 * self.err_zz
        for (t, env, dg, d32, due, mh, mz) in self.disagree:
            other = d32 if dg == -1 else dg                       # the side that does not report a failure must hold what is due without one
            ok = (dg == -1) != (d32 == -1) and other == (1.0 if due else 0.0) and (mh < bound_h or mz < bound_z)
            assert ok, (f"{lab}DONE at step {t}, env {env}: {dg} against the oracle's {d32} (time-out due: {due}); margins height {mh:.2e} (bound {bound_h:.2e}), "
                        f"tilt {mz:.2e} (bound {bound_z:.2e}). The tilt margin is the record's, one substep before the quaternion the flag is decided on "
                        f"(record_tilt_zz): a lone tilt failure against a running / timed-out row with the height far from its threshold can be a rounding "
                        f"flip on the tilt threshold that this margin cannot see - check the integrated state's margin before suspecting the kernel")
        assert len(self.disagree) <= self.max_exempt, f"{lab}{len(self.disagree)} DONE flags on a threshold differ from the oracle's: {self.disagree}"
        out = dict(counts=dict(self.counts), max_episode=self.max_episode, reset_rows=self.reset_rows, margin_height=self.margin_height, margin_zz=self.margin_zz,
                   bound_height=bound_h, bound_zz=bound_z, reset_err=dict(self.reset_err), oracle_reset_err=dict(self.o32_reset_err), exempted=len(self.disagree), record={})
        if self.terminal:
            out["record"] = check_record_against_oracle_spread(self.rec_got, self.rec_o32, np.concatenate(self.terminal), np.concatenate(self.switch), label=lab)
        if verbose:
            print(f"{lab}episode ends:", out)
        return out


MIN_TERMINAL_ROWS = 100       # below this a sample carries no 99th percentile of its own


def check_record_against_oracle_spread(err_got: dict, err_o32: dict, terminal: np.ndarray, switch: np.ndarray, label=""):
    """The completed aux_t rows by column group (AUX_RECORD_GROUPS), by the rule of check_against_oracle_spread: error against the fp64
    oracle beside the fp32 oracle's own error on the SAME env-steps, terminal rows (the record of a finished episode, which must hold the
    state BEFORE the reset) apart from running rows:
      * median and p99 at most 2x the oracle's, floored at a few fp32 roundings of the quantity;
      * terminal rows: the extreme value within 2x the oracle's own extreme (same floor) - no solver switch excuses a wrong record there.
        Where a run has fewer than MIN_TERMINAL_ROWS terminal rows (the 5 of the default-config case), their own quantiles are no
        yardstick: a p99 is the extreme of anything under 100 samples, and the ratio of two such extremes is not a stable statistic. Only
        there, the oracle's quantile over ALL rows of the run stands in where it is the larger, and its p99 for the extreme: a terminal
        record is written before the reset, from the same arithmetic as a running one;
      * running rows: no heavier tail than the oracle's - the env-steps beyond 2x the oracle's p99.9 number at most 1.5x the oracle's own
        count + 5, and at most 8 of them on env-steps the oracle does not flag as sitting on a discrete switch of the solver.
    Returns {group: {"terminal" / "running": (n, p50, p99, max, oracle p50, oracle p99, oracle max)}}."""
    out = {}
    for name, (_, _, floor) in AUX_RECORD_GROUPS.items():
        hh, oo = np.concatenate(err_got[name]), np.concatenate(err_o32[name])
        out[name] = {}
        for rows, where in ((terminal, "terminal"), (~terminal, "running")):
            h, o = hh[rows], oo[rows]
            if h.size == 0:
                continue
            out[name][where] = (int(h.size),) + tuple(float(f"{x:.3g}") for x in (np.median(h), np.quantile(h, 0.99), h.max(), np.median(o), np.quantile(o, 0.99), o.max()))
            few = where == "terminal" and h.size < MIN_TERMINAL_ROWS
            for qn, q in (("median", 0.5), ("p99", 0.99)):
                hq, oq = np.quantile(h, q), max(np.quantile(o, q), np.quantile(oo, q) if few else 0.0)
                assert hq <= 2 * max(oq, floor), f"{label}aux_t {name} {where} rows {qn}: {hq:.3e} vs oracle fp32 {oq:.3e}"
            if where == "terminal":
                omax = max(o.max(), np.quantile(oo, 0.99) if few else 0.0)
                assert h.max() <= 2 * max(omax, floor), f"{label}aux_t {name} terminal rows max: {h.max():.3e} vs oracle fp32 {omax:.3e} (env-step {int(np.nonzero(rows)[0][h.argmax()])})"
            else:
                thr = 2 * max(np.quantile(o, 0.999), floor)
                nh, no = int((h > thr).sum()), int((o > thr).sum())
                assert nh <= 1.5 * no + 5, f"{label}aux_t {name} running rows: {nh} env-steps beyond {thr:.2e}, the oracle's fp32 run has {no}"
                unexplained = int(((h > thr) & ~switch[rows]).sum())
                assert unexplained <= 8, f"{label}aux_t {name} running rows: {unexplained} outliers beyond {thr:.2e} without a discrete solver switch"
    return out


def teacher_forced_config(N, command):
    """kbj_config of a case of test_teacher_forced_steps_match_oracle: `command` names a case of EPISODE_END_CASES, or the command source
    ("sampler"; "fixed": BASELINE configs[1], command_mode 1, (0.5, 0, 0); "sampler on jax.random keys": command_mode 2)."""
    from kbot_joystick_amd.spec import layout as L
    kw = dict(EPISODE_END_CASES[command]["cfg"]) if command in EPISODE_END_CASES else {}
    if command == "fixed":
        kw = dict(command_mode=1, fixed_command=[0.5] + [0.0] * 15)
    if command == "sampler on jax.random keys":
        kw = dict(command_mode=2, switch_prob=0.2)
    return L.default_config(num_envs=N, batch_size=min(512, N), **kw)


def oracle_pair_step(o, o64, act, aux_in):
    """One teacher-forced control step of the fp32 oracle `o` and, from the same state, of the fp64 oracle `o64`. Returns (ep0, es0, Step fp32,
    Step fp64, switch): the start state, both results and the env-steps on which the two evaluations differ in the solver's discrete state
    (active contacts / force-carrying rows / iteration counts, or the iteration cap bites)."""
    ep0, es0 = o.ep.copy(), o.es.copy()
    o64.ep[:], o64.es[:] = ep0, es0
    x32, x64 = aux_in.copy(), aux_in.copy()
    a64, c64, n64, d64 = o64.step_diag(act, x64)
    a32, c32, n32, d32 = o.step_diag(act, x32)
    it = o.config.solver_iterations
    switch = (d32 != d64).any(1) | (d64[:, 0] >= it) | (d32[:, 0] >= it)
    return ep0, es0, Step(o.ep.copy(), o.es.copy(), x32, a32, c32, n32), Step(o64.ep.copy(), o64.es.copy(), x64, a64, c64, n64), switch


def emu_stepper(model, cfg, seed, lib=None):
    """The host emulation of the kernel body (tests/emu) as `step(ep0, es0, act, aux_in) -> Step`."""
    emu = lib or emu_lib()
    N = cfg.num_envs

    def step(ep0, es0, act, aux_in):
        from kbot_joystick_amd.spec import layout as L
        ep, es, x = ep0.copy(), es0.copy(), aux_in.copy()
        a, c, n = np.zeros((N, L.LD_ACTOR), np.float32), np.zeros((N, L.LD_CRITIC), np.float32), np.zeros((N, L.AUX["SIZE"]), np.float32)
        emu.kbj_emu_env_step(C.byref(model), C.byref(cfg), C.c_uint32(seed), fptr(ep), fptr(es), fptr(np.ascontiguousarray(act, np.float32)), fptr(x), fptr(a), fptr(c), fptr(n))
        return Step(ep, es, x, a, c, n)
    return step


def episode_end_run(model, case: str, stepper_factory=None, seed=11, verbose=True):
    """A case of EPISODE_END_CASES, teacher-forced: the fp32 oracle's state goes into the fp64 oracle and into `stepper_factory(cfg, seed)`'s
    implementation before every step. Returns (EpisodeEndAudit.finish()'s figures, the audit)."""
    from oracle import oracle as O
    spec = EPISODE_END_CASES[case]
    N = spec["N"]
    cfg = teacher_forced_config(N, case)
    o, o64 = O.Oracle(model, cfg, seed=seed, precision="f32"), O.Oracle(model, cfg, seed=seed, precision="f64")
    _, _, x0 = o.reset_all()
    step = stepper_factory(cfg, seed) if stepper_factory else None
    rng = np.random.default_rng(0)
    audit = EpisodeEndAudit(cfg, label=case + ": ")
    for t in range(spec["steps"]):
        act = random_actions(model, rng, N)
        ep0, es0, s32, s64, switch = oracle_pair_step(o, o64, act, x0)
        audit.add(es0, s32, s64, step(ep0, es0, act, x0) if step else None, switch)
        x0 = s32.aux
    return audit.finish(spec["floors"], verbose=verbose), audit


# ---------------------------------------------------------------------------------------------------------------------
# actor-critic / PPO side: the synthetic minibatch problem of tests/test_gpu_nn.py as CPU tensors, so that the oracle half of a
# parity test (and the CPU-only liveness checks of tests/test_oracle_nn.py) needs no device
# ---------------------------------------------------------------------------------------------------------------------
# The update's hyperparameters at non-default values (tests/test_gpu_hparams.py; liveness on the oracle alone in tests/test_oracle_nn.py).
# name -> kbj_config overrides. Each case must move the oracle's gradient by >= 1e-2 of its norm (100x the parity bound): measured on
# the CPU at both shapes below, the smallest is 3.2e-2 (value_clip 0.05); the table is in tests/test_oracle_nn.py.
HPARAM_CASES = {
    "entropy_coef=0.5": dict(entropy_coef=0.5),
    "value_loss_coef=2": dict(value_loss_coef=2.0),
    "clip_param=0.05": dict(clip_param=0.05),
    "clip_param=0.6": dict(clip_param=0.6),
    "value_clip=0.05": dict(value_clip=0.05),
    "value_clip=5": dict(value_clip=5.0),
    "log_ratio_clip=0.25": dict(log_ratio_clip=0.25),
    "adv_eps=0.5": dict(adv_eps=0.5),
    "max_std=0.35": dict(max_std=0.35),
    "min_std=0.2": dict(min_std=0.2),
    "var_scale=1.5": dict(var_scale=1.5),       # pushes 78 % / 97 % of the std elements into the default max_std = 1 clamp ...
    "var_scale=0.25": dict(var_scale=0.25),     # ... so a second value that stays below it: the scale's own gradient factor on every element
    "lpf_alpha=1": dict(lpf_alpha=1.0),
    "lpf_alpha=0.1": dict(lpf_alpha=0.1),
    "gamma=0": dict(gamma=0.0),
    "gamma=1,lam=1": dict(gamma=1.0, lam=1.0),
    "lam=0": dict(lam=0.0),
    "combined": dict(entropy_coef=0.1, value_loss_coef=1.5, clip_param=0.1, value_clip=0.1, log_ratio_clip=0.4, adv_eps=0.1, max_std=0.6,
                     min_std=0.05, var_scale=0.8, lpf_alpha=0.3, gamma=0.9, lam=0.8),
}
HPARAM_HEAD_CASES = ["max_std=0.35", "min_std=0.2", "var_scale=1.5", "var_scale=0.25", "lpf_alpha=1", "lpf_alpha=0.1"]     # the fields the forward-only passes read
# (H, N, B, T): one small and ragged; one at H = 256 whose 12 steps cross the 10-step fetch chunks of the head's time scans
HPARAM_SHAPES = [(64, 40, 32, 9), (256, 40, 32, 12)]


# ---- the counter generator behind the action and init streams (kbj_model.h KBJ_RNG_ACTION, KBJ_RNG_INIT), vectorised ----
RNG_ACTION, RNG_INIT = RNG["ACTION"], RNG["INIT"]
# tools/head_check: the largest E_Z of its table (max of the derivable 2.16e-6 and 4 x the host fp32 restatement's error over a case's draws);
# the device's worst |z - z_ref| measured against it is in EXPERIMENTS.md
Z_BOUND = 3.3e-6


def threefry_np(k0, k1, c0, c1):
    """threefry2x32-20 (Salmon et al., SC'11) over broadcast integer arrays, every word taken mod 2^32: (x0, x1) as uint64 arrays below 2^32.
    Pinned to oracle.threefry (itself pinned to the Random123 known answers) by tests/test_oracle_physics.py."""
    M = np.uint64(0xFFFFFFFF)
    k0, k1, c0, c1 = np.broadcast_arrays(*(np.asarray(v).astype(np.uint64) & M for v in (k0, k1, c0, c1)))
    ks = (k0, k1, k0 ^ k1 ^ np.uint64(0x1BD11BDA))
    x0, x1 = (c0 + ks[0]) & M, (c1 + ks[1]) & M
    rot = (13, 15, 26, 6, 17, 29, 16, 24)
    for g in range(5):
        for r in range(4):
            n = np.uint64(rot[(g & 1) * 4 + r])
            x0 = (x0 + x1) & M
            x1 = (((x1 << n) | (x1 >> (np.uint64(32) - n))) & M) ^ x0
        x0 = (x0 + ks[(g + 1) % 3]) & M
        x1 = (x1 + ks[(g + 2) % 3] + np.uint64(g + 1)) & M
    return x0, x1


def stream_key(seed, stream):
    return (int(seed) ^ (stream * 0x9E3779B9)) & 0xFFFFFFFF


def z_ref(seed, env, step, joint):
    """The action stream's Gaussian draw from the exact threefry words, radius and cosine in double: key (seed ^ stream, env), counter
    (step, joint); u1 = ((b0 >> 8) + 1) / 2^24 and u2 = (b1 >> 8) / 2^24 are exact in fp32, the angle is the fp32 constant's product."""
    b0, b1 = threefry_np(stream_key(seed, RNG_ACTION), env, step, joint)
    u1, u2 = ((b0 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 2 ** 24, (b1 >> np.uint64(8)).astype(np.float64) / 2 ** 24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(float(np.float32(6.283185307179586)) * u2)


def init_uniform_ref(seed, leaf, n, fan_in):
    """init_uniform_kernel bit for bit: element i of leaf `leaf` is fmaf(2 b, u, -b) with b = 1 / sqrtf(fan_in) and u = (b0 >> 8) / 2^24 of
    threefry(key (seed ^ stream, leaf), counter (i >> 32, i)). b = mb 2^(e - 24) and u = k 2^-24 make the exact value the integer
    mb (2 k - 2^24) (below 2^49: exact in int64) times 2^(e - 48); the one rounding of the fma is the int64 -> float32 conversion."""
    b = np.float32(1.0) / np.sqrt(np.float32(fan_in))
    m, e = np.frexp(b)
    mb = int(m * 2 ** 24)
    i = np.arange(n, dtype=np.uint64)
    b0, _ = threefry_np(stream_key(seed, RNG_INIT), leaf, i >> np.uint64(32), i)
    k = (b0 >> np.uint64(8)).astype(np.int64)
    return np.ldexp((mb * (2 * k - 2 ** 24)).astype(np.float32), int(e) - 48)


def init_params_ref(H, seed, depth=2, extra_obs=(0, 0)):
    """kbj_init_params bit for bit as [(leaf name, offset, values)]: the leaves in the order of oracle.nn.param_shapes, numbered from 0, laid
    out back to back; fan-in = the input projection's width for its weight and bias, the hidden size for every other leaf."""
    from oracle import nn as ON
    out, off = [], 0
    for leaf, (name, shp) in enumerate(ON.param_shapes(H, depth, extra_obs)):
        nin = (ON.NOBS_ACTOR + extra_obs[0]) if name.startswith("actor") else (ON.NOBS_CRITIC + extra_obs[1])
        n = int(np.prod(shp))
        out.append((name, off, init_uniform_ref(seed, leaf, n, nin if ".input_proj." in name else H)))
        off += n
    return out


def init_like_params(H, seed, depth=2):
    """A CPU draw from the distribution of kbj_init_params (uniform +-1/sqrt(fan_in) per leaf; not its stream: init_params_ref above follows
    the stream): fp64 flat vector."""
    import torch
    from oracle import nn as ON
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for name, shp in ON.param_shapes(H, depth):
        fan_in = shp[1] if name.endswith("input_proj.weight") else (ON.NOBS_ACTOR if name == "actor.input_proj.bias" else ON.NOBS_CRITIC if name == "critic.input_proj.bias" else H)
        out.append((torch.rand(int(np.prod(shp)), generator=g, dtype=torch.float64) * 2 - 1) / np.sqrt(fan_in))
    return torch.cat(out)


def synthetic_arrays(N, T, H, seed=0, depth=2, mirror=False):
    """The synthetic trajectory of the PPO parity tests as CPU float32 tensors (rows padded as the device rows are): name -> tensor."""
    import torch
    from kbot_joystick_amd.spec import layout as L
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = dict(actor_obs=torch.zeros(T + 1, N, L.LD_ACTOR), critic_obs=torch.zeros(T + 1, N, L.LD_CRITIC))
    a["actor_obs"][:, :, :65] = torch.randn(T + 1, N, 65, generator=g) * 0.5
    a["critic_obs"][:, :, :475] = torch.randn(T + 1, N, 475, generator=g) * 0.5
    a["action"] = torch.randn(T, N, 20, generator=g) * 0.3
    a["done"] = (torch.rand(T, N, generator=g) < 0.15).float() * torch.where(torch.rand(T, N, generator=g) < 0.5, -1.0, 1.0)
    a["reward"] = torch.rand(T, N, generator=g)
    a["carry0_actor_hc"] = torch.randn(depth, 2, N, H, generator=g) * 0.3
    a["carry0_critic_hc"] = torch.randn(depth, 2, N, H, generator=g) * 0.3
    a["carry0_lpf"] = torch.randn(N, 20, generator=g) * 0.2
    if mirror:
        a["carry0_actor_mirror_hc"] = torch.randn(depth, 2, N, H, generator=g) * 0.3
        a["carry0_critic_mirror_hc"] = torch.randn(depth, 2, N, H, generator=g) * 0.3
        a["carry0_lpf_mirror"] = torch.randn(N, 20, generator=g) * 0.2
    return a


def fill_traj(tr, arr):
    """Copy synthetic_arrays() into a TrajBuffers of the same shape."""
    from kbot_joystick_amd.spec import layout as L
    T = tr.T
    tr.actor_obs.copy_(arr["actor_obs"]); tr.critic_obs.copy_(arr["critic_obs"])
    tr.action.copy_(arr["action"])
    tr.aux[:T, :, L.AUX["DONE"]] = arr["done"].to(tr.aux.device)
    tr.reward.copy_(arr["reward"])
    for k in ("carry0_actor_hc", "carry0_critic_hc", "carry0_lpf", "carry0_actor_mirror_hc", "carry0_critic_mirror_hc", "carry0_lpf_mirror"):
        if k in arr:
            getattr(tr, k).copy_(arr[k])
    for k in ("logp", "value"):
        if k in arr:
            getattr(tr, k).copy_(arr[k])


def _carry(arr, key, ii, depth):
    c = arr[key].double()
    return [[c[l, k] if ii is None else c[l, k][ii] for k in range(2)] for l in range(depth)]


def oracle_head_series(p, cfg, jb, arr, ii=None, depth=2):
    """The actor head over the trajectory on the oracle (no gradient): (filtered mean [T,B,20], std [T,B,20]) for the envs `ii` (None: all)."""
    import torch
    from oracle import nn as ON
    T = arr["action"].shape[0]
    sel = (lambda x: x) if ii is None else (lambda x: x[:, ii])
    ao, done = sel(arr["actor_obs"][:T].double()), sel(arr["done"].double())
    ca, lpf = _carry(arr, "carry0_actor_hc", ii, depth), (arr["carry0_lpf"].double() if ii is None else arr["carry0_lpf"].double()[ii])
    means, stds = [], []
    with torch.no_grad():
        for t in range(T):
            out_a, ca = ON.net_forward(p, "actor", ao[t], ca, depth)
            mean, std, lpf = ON.actor_head(out_a, ao[t], lpf, jb, cfg)
            means.append(mean); stds.append(std)
            keep = (done[t] == 0).double()[:, None]
            ca = [[h * keep, c * keep] for h, c in ca]
            lpf = lpf * keep
    return torch.stack(means), torch.stack(stds)


def oracle_old_policy(cfg, jb, p64, arr, H, g, depth=2):
    """Old log-probs / values of the synthetic problem: the oracle's own under `cfg` plus N(0, 0.3) noise drawn from `g` (so that some
    ratios leave the clip range), rounded to the float32 the device arrays hold. Returns (logp_old, value_old, (lp, v, en) noise-free)."""
    import torch
    from oracle import nn as ON
    T, N = arr["action"].shape[:2]
    with torch.no_grad():
        lp, v, en, *_ = ON.ppo_variables(ON.unflatten(p64, H, depth), cfg, jb, arr["actor_obs"][:T].double(), arr["critic_obs"][:T].double(), arr["action"].double(),
                                         arr["done"].double(), _carry(arr, "carry0_actor_hc", None, depth), _carry(arr, "carry0_critic_hc", None, depth),
                                         arr["carry0_lpf"].double(), depth)
    logp_old = (lp + 0.3 * torch.randn(T, N, generator=g).double()).float()
    value_old = (v + 0.3 * torch.randn(T, N, generator=g).double()).float()
    return logp_old, value_old, (lp, v, en)


def oracle_minibatch_grad(cfg, jb, p64, arr, idx, H, adv, target, adv_sums=None, depth=2, dtype=None):
    """Autograd of ON.ppo_loss(ON.ppo_variables(...)) over the minibatch `idx` of the synthetic problem; arr["logp"] / arr["value"] are the old
    policy's, adv / target [T, N]. dtype: torch.float32 reruns the same loss in fp32. Returns (flat gradient, metrics dict of floats, logp)."""
    import torch
    from oracle import nn as ON
    dt = dtype or torch.float64
    T = arr["action"].shape[0]
    ii = idx.long()
    pf = p64.to(dt).clone().requires_grad_(True)
    sel = lambda x: x.to(dt)[:, ii]
    cst = lambda c: [[x.to(dt) for x in hc] for hc in c]
    lp, v, en, *_ = ON.ppo_variables(ON.unflatten(pf, H, depth), cfg, jb.to(dt), sel(arr["actor_obs"][:T]), sel(arr["critic_obs"][:T]), sel(arr["action"]), sel(arr["done"]),
                                     cst(_carry(arr, "carry0_actor_hc", ii, depth)), cst(_carry(arr, "carry0_critic_hc", ii, depth)), arr["carry0_lpf"].to(dt)[ii], depth)
    loss, mt = ON.ppo_loss(cfg, lp, v, en, sel(arr["logp"]), sel(arr["value"]), sel(adv), sel(target), adv_sums=adv_sums)
    loss.backward()
    return pf.grad.double(), {k: float(x.detach()) for k, x in mt.items()}, lp.detach().double()


METRIC_NAMES = ["loss", "policy", "value", "entropy", "clipfrac", "kl", "adv_mean", "adv_std"]


def hparam_problem(cfg, jb, p64, arr, H, N, B):
    """The synthetic minibatch problem under `cfg` on the oracle alone: the minibatch indices, the old policy drawn under `cfg`, GAE with
    cfg's gamma / lambda, the fp64 autograd gradient and what the liveness conditions need. Returns a dict; arr gains "logp" / "value"."""
    import torch
    from oracle import nn as ON
    g = torch.Generator(device="cpu").manual_seed(5)
    idx = torch.randperm(N, generator=g)[:B].int()
    arr = dict(arr)
    arr["logp"], arr["value"], _ = oracle_old_policy(cfg, jb, p64, arr, H, g)
    adv, tgt = ON.gae(arr["value"].double(), arr["reward"].double(), arr["done"].double(), cfg.gamma, cfg.lam)
    grad, mt, lp = oracle_minibatch_grad(cfg, jb, p64, arr, idx, H, adv, tgt)
    _, std = oracle_head_series(ON.unflatten(p64, H), cfg, jb, arr, idx.long())
    dlp = (lp - arr["logp"].double()[:, idx.long()]).abs()
    return dict(arr=arr, idx=idx, adv=adv, target=tgt, grad=grad, metrics=mt,
                frac_beyond_lrclip=float((dlp >= cfg.log_ratio_clip).double().mean()), frac_std_clamped=float((std >= cfg.max_std).double().mean()))


def check_hparam_liveness(name, cfg, case, default):
    """The conditions that make a hyperparameter case a test of its term (tests/test_gpu_hparams.py): asserted, not measured."""
    diff = float((case["grad"] - default["grad"]).norm() / case["grad"].norm())
    assert diff >= 1e-2, (name, "the override moves the oracle's gradient by only", diff)
    assert 0.02 < case["metrics"]["clipfrac"] < 0.98, (name, case["metrics"]["clipfrac"])
    if abs(cfg.log_ratio_clip - 10.0) > 1e-6:
        assert case["frac_beyond_lrclip"] >= 0.10, (name, case["frac_beyond_lrclip"])
    if abs(cfg.max_std - 1.0) > 1e-6:
        assert 0.10 <= case["frac_std_clamped"] <= 0.90, (name, case["frac_std_clamped"])
    return diff


def check_grad_parity(gg, go, H, depth=2, label=""):
    """The gradient bounds of tests/test_gpu_nn.py: per leaf max error / leaf max < 2e-3, global relative L2 < 1e-4. Returns the two worst figures."""
    from oracle import nn as ON
    off, worst = 0, 0.0
    for name, shp in ON.param_shapes(H, depth):
        n = int(np.prod(shp))
        a, b = gg[off:off + n], go[off:off + n]
        err = float((a - b).abs().max() / (b.abs().max() + 1e-12))
        worst = max(worst, err)
        assert err < 2e-3, (label, name, err, float(b.abs().max()))
        off += n
    assert off == go.numel()
    rel = float((gg - go).norm() / go.norm())
    assert rel < 1e-4, (label, rel)
    return worst, rel


def check_metrics_parity(mg, mt, label=""):
    """metrics[0..7] of kbj_ppo_grad against the oracle's dict: 2e-4 * (1 + |x|)."""
    worst = 0.0
    for k, name in enumerate(METRIC_NAMES):
        e = abs(float(mg[k]) - mt[name])
        worst = max(worst, e / (1 + abs(mt[name])))
        assert e < 2e-4 * (1 + abs(mt[name])), (label, name, float(mg[k]), mt[name])
    return worst
