"""Host restatements of kbj_env_perturb and kbj_robustness (include/kbj.h, word for word), and the dynamics cases the perturbation tests share.

perturbed_row: float32 numpy, one product or one sum per written word (numpy never contracts), so the device's words are reproduced bit for
bit. robustness_ref: sequential float64 loops in row order, then in env order."""
import numpy as np

from kbot_joystick_amd.spec import layout as L

EP, P, R, S, TE = L.EP, L.PERT, L.RREC, L.RSTAT, L.TERR
f32 = np.float32

# the columns kbj_env_perturb writes whatever the record holds (LATENCY: only for a record word >= 0), and those it never touches
WRITTEN = np.zeros(EP["SIZE"], bool)
WRITTEN[:EP["JPBIAS"]] = True
WRITTEN[EP["MU"]] = True
KEPT = ~WRITTEN
KEPT[EP["LATENCY"]] = False
# the columns each knob owns (record slot -> EP columns)
OWN = dict(MASS_SCALE=list(range(EP["MASS"], EP["ARMATURE"])), MU_SCALE=[EP["MU"]], ARMATURE_SCALE=list(range(EP["ARMATURE"], EP["FRICLOSS"])),
           FRICLOSS_SCALE=list(range(EP["FRICLOSS"], EP["CAP_POS"])), LATENCY=[EP["LATENCY"]], KP_SCALE=list(range(EP["KP"], EP["KD"])),
           KD_SCALE=list(range(EP["KD"], EP["TAULIM"])), TAULIM_SCALE=list(range(EP["TAULIM"], EP["ACTBIAS"])), ACTBIAS=list(range(EP["ACTBIAS"], EP["JPBIAS"])))


def identity_record() -> np.ndarray:
    rec = np.zeros(P["SIZE"], f32)
    for k in ("MASS_SCALE", "MU_SCALE", "ARMATURE_SCALE", "FRICLOSS_SCALE"):
        rec[P[k]] = 1
    for k in ("KP_SCALE", "KD_SCALE", "TAULIM_SCALE"):
        rec[P[k]:P[k] + L.NU] = 1
    rec[P["LATENCY"]] = -1
    return rec


def record_valid(rec) -> bool:
    """The "valid" column of kbj_model.h KBJ_PERT_*: every word read is finite (the spare words are not read), scales positive (KD, FRICLOSS:
    not negative), the payload not negative, the latency negative or whole."""
    rec = np.asarray(rec, f32)
    read = np.ones(P["SIZE"], bool)
    read[P["SPARE"]:P["KP_SCALE"]] = False
    if not np.isfinite(rec[read]).all():
        return False
    pos = [P["MASS_SCALE"], P["MU_SCALE"], P["ARMATURE_SCALE"]] + list(range(P["KP_SCALE"], P["KD_SCALE"])) + list(range(P["TAULIM_SCALE"], P["ACTBIAS"]))
    nonneg = [P["PAYLOAD"], P["FRICLOSS_SCALE"]] + list(range(P["KD_SCALE"], P["TAULIM_SCALE"]))
    lat = rec[P["LATENCY"]]
    return bool((rec[pos] > 0).all() and (rec[nonneg] >= 0).all() and (lat < 0 or lat == np.floor(lat)))


def perturbed_row(model, record, row) -> np.ndarray:
    """The KBJ_EP row kbj_env_perturb leaves for a masked env whose row was `row` and whose record is `record`: float32 throughout. An
    invalid record returns `row` unchanged."""
    rec, out = np.asarray(record, f32), np.array(row, f32, copy=True)
    if not record_valid(rec):
        return out
    arr = lambda x: np.array(x, f32)
    torso = int(model.torso_body)
    shift = np.zeros((L.NBODY, 3), f32)
    shift[torso] = rec[P["COM_SHIFT"]:P["COM_SHIFT"] + 3]
    out[EP["IPOS"]:EP["MASS"]] = (arr(model.body_ipos) + shift).reshape(-1)
    mass = arr(model.body_mass) * rec[P["MASS_SCALE"]]
    mass[torso] = mass[torso] + rec[P["PAYLOAD"]]
    out[EP["MASS"]:EP["INERTIA"]] = mass
    out[EP["INERTIA"]:EP["ARMATURE"]] = (arr(model.body_inertia) * rec[P["MASS_SCALE"]]).reshape(-1)
    out[EP["ARMATURE"]:EP["FRICLOSS"]] = arr(model.dof_armature) * rec[P["ARMATURE_SCALE"]]
    out[EP["FRICLOSS"]:EP["CAP_POS"]] = arr(model.dof_frictionloss) * rec[P["FRICLOSS_SCALE"]]
    out[EP["CAP_POS"]:EP["CAP_HALF"]] = (arr(model.cap_pos) + f32(0)).reshape(-1)
    out[EP["CAP_HALF"]:EP["CAP_RAD"]] = arr(model.cap_halflen)
    out[EP["CAP_RAD"]:EP["KP"]] = arr(model.cap_radius)
    out[EP["KP"]:EP["KD"]] = arr(model.kp) * rec[P["KP_SCALE"]:P["KP_SCALE"] + L.NU]
    out[EP["KD"]:EP["TAULIM"]] = arr(model.kd) * rec[P["KD_SCALE"]:P["KD_SCALE"] + L.NU]
    out[EP["TAULIM"]:EP["ACTBIAS"]] = arr(model.tau_limit) * rec[P["TAULIM_SCALE"]:P["TAULIM_SCALE"] + L.NU]
    out[EP["ACTBIAS"]:EP["JPBIAS"]] = rec[P["ACTBIAS"]:P["ACTBIAS"] + L.NU]
    if rec[P["LATENCY"]] >= 0:
        out[EP["LATENCY"]] = rec[P["LATENCY"]]
    out[EP["MU"]] = f32(model.contact_mu) * rec[P["MU_SCALE"]]
    assert out.dtype == f32
    return out


def perturbed_rows(model, records, rows, mask=None) -> np.ndarray:
    """perturbed_row per env; envs whose mask entry is zero keep their row."""
    return np.stack([perturbed_row(model, r, x) if mask is None or mask[i] != 0 else np.array(x, f32) for i, (r, x) in enumerate(zip(records, rows))])


def status_ref(records, mask=None) -> np.ndarray:
    return np.array([0 if mask is not None and mask[i] == 0 else (1 if record_valid(r) else -1) for i, r in enumerate(records)], np.int32)


def robustness_ref(done, err, group, G):
    """kbj_robustness restated: done [T, N] (the DONE column), err [T, N, TERR SIZE] float32, group None or [N] ints, G groups ->
    (rec [N, RREC SIZE], stats [G, RSTAT SIZE]), float64, sums sequential in row order and then in env order."""
    rec = scan_ref(done, err)
    return rec, group_ref(rec, group, G)


def scan_ref(done, err) -> np.ndarray:
    """Stage 1: one env's rows in ascending order."""
    T, N = done.shape
    rec = np.zeros((N, R["SIZE"]), np.float64)
    with np.errstate(invalid="ignore"):
        for n in range(N):
            r = rec[n]
            r[R["FIRST_FALL"]] = -1.0
            r[R["ERR_MAX"]:R["ERR_MAX"] + L.NTERR] = -1.0
            for t in range(T):
                r[R["ROWS"]] += 1
                if done[t, n] < 0:
                    r[R["FALLS"]] += 1
                    if r[R["FIRST_FALL"]] < 0:
                        r[R["FIRST_FALL"]] = t
                if done[t, n] > 0:
                    r[R["TIMEOUTS"]] += 1
                if err[t, n, TE["SETTLED"]] != 0:
                    r[R["SETTLED"]] += 1
                    for k in range(L.NTERR):
                        e = err[t, n, k]
                        x = np.float64(e)
                        r[R["ERR_SUM"] + k] += x
                        r[R["ERR_SUMSQ"] + k] += x * x
                        if x > r[R["ERR_MAX"] + k]:
                            r[R["ERR_MAX"] + k] = x
    return rec


def group_ref(rec, group, G) -> np.ndarray:
    """Stage 2: a group's envs in env order."""
    N = rec.shape[0]
    with np.errstate(invalid="ignore"):
        stats = np.zeros((G, S["SIZE"]), np.float64)
        stats[:, S["FIRST_FALL_MIN"]] = -1.0
        stats[:, S["ERR_MAX"]:S["ERR_MAX"] + L.NTERR] = -1.0
        for n in range(N):
            g = 0 if group is None else int(group[n])
            if not 0 <= g < G:
                continue
            s, r = stats[g], rec[n]
            s[S["ENVS"]] += 1
            s[S["FALLS"]] += r[R["FALLS"]]; s[S["TIMEOUTS"]] += r[R["TIMEOUTS"]]; s[S["ROWS"]] += r[R["ROWS"]]; s[S["SETTLED"]] += r[R["SETTLED"]]
            ff = r[R["FIRST_FALL"]]
            if ff >= 0:
                s[S["FELL_ENVS"]] += 1
                s[S["FIRST_FALL_SUM"]] += ff
                if s[S["FIRST_FALL_MIN"]] < 0 or ff < s[S["FIRST_FALL_MIN"]]:
                    s[S["FIRST_FALL_MIN"]] = ff
            for k in range(L.NTERR):
                s[S["ERR_SUM"] + k] += r[R["ERR_SUM"] + k]
                s[S["ERR_SUMSQ"] + k] += r[R["ERR_SUMSQ"] + k]
                if r[R["ERR_MAX"] + k] > s[S["ERR_MAX"] + k]:
                    s[S["ERR_MAX"] + k] = r[R["ERR_MAX"] + k]
    return stats


def same_words(got, want) -> bool:
    """Bit for bit, except that where the restatement's word is a NaN the device's is a NaN (a NaN's payload is the adder's own)."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    return got.shape == want.shape and bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def groups(N, G, seed=5) -> np.ndarray:
    """[N] int32 groups in [-1, G]: both ends are outside, so some envs are in no group."""
    return np.random.default_rng(seed + 31 * N + G).integers(-1, G + 1, N).astype(np.int32)


def synthetic(T, N, seed=3):
    """(aux [T + 1, N, AUX SIZE], err [T, N, TERR SIZE]) float32 for kbj_robustness: DONE draws -1, 0, 1 and values that are not whole; errors
    of mixed scale with NaNs and negative values among them; every fourth env without a settled row, every fifth without a fall; SETTLED flags 0, 1 and 2."""
    rng = np.random.default_rng(seed + 1000 * T + N)
    aux = rng.standard_normal((T + 1, N, L.AUX["SIZE"])).astype(f32)
    aux[..., L.AUX["DONE"]] = rng.choice(np.array([-1, 0, 0, 0, 0, 0, 1, -0.5, 2.5], f32), (T + 1, N), p=[0.05, 0.5, 0.1, 0.1, 0.1, 0.05, 0.05, 0.025, 0.025])
    never = aux[:, 1::5, L.AUX["DONE"]]
    never[never < 0] = 0                                                               # every fifth env never falls
    err = (np.abs(rng.standard_normal((T, N, TE["SIZE"]))) * 10.0 ** rng.integers(-3, 3, (T, N, TE["SIZE"]))).astype(f32)
    err[..., :L.NTERR][rng.random((T, N, L.NTERR)) < 0.02] = np.nan
    err[..., :L.NTERR][rng.random((T, N, L.NTERR)) < 0.02] *= -1
    err[..., TE["SETTLED"]] = rng.choice(np.array([0, 1, 2], f32), (T, N), p=[0.3, 0.6, 0.1])
    err[:, ::4, TE["SETTLED"]] = 0
    if N > 2:
        err[:, 2, :L.NTERR] = np.abs(np.nan_to_num(err[:, 2, :L.NTERR], nan=1.0))       # one env whose sums stay finite
        err[:, 2, TE["SETTLED"]] = 1
    return aux, err


# ---- the dynamics cases: the identity and seven perturbations, 8 envs each at N = 64 ----
def dynamics_cases() -> list:
    from kbot_joystick_amd.host.robustness import Perturbation as Pn
    return [Pn("nominal"), Pn("friction x0.3", friction_scale=0.3), Pn("mass x1.3", mass_scale=1.3), Pn("payload 8 kg", payload_kg=8.0), Pn("kp x0.6", kp_scale=0.6),
            Pn("torque x0.5", torque_scale=0.5), Pn("latency 5", latency_substeps=5), Pn("armature x2, latency 0", armature_scale=2.0, latency_substeps=0)]


def dynamics_records(N=64) -> np.ndarray:
    """[N, PERT SIZE]: env e runs case e % 8, as the sweep deals its cases."""
    cases = dynamics_cases()
    return np.stack([cases[e % len(cases)].record() for e in range(N)])


DYN_N, DYN_STEPS, DYN_SEED = 64, 20, 11


def dynamics_liveness(model):
    """{case name: [8] per-env figure}: through the teacher-forced loop of dynamics_run, at every step the fp64 oracle under the perturbed rows
    against a nominal twin (the identity record's rows) stepped once from the SAME state with the same action: per env the largest |qvel
    difference| over any dof and any of the DYN_STEPS steps (steps that end an episode in either are left out). Also returns the latencies
    the reset drew."""
    from oracle import oracle as Or
    from tests import helpers as H
    N = DYN_N
    cfg = H.teacher_forced_config(N, "sampler")
    o, o64, twin = (Or.Oracle(model, cfg, seed=DYN_SEED, precision=p) for p in ("f32", "f64", "f64"))
    _, _, x0 = o.reset_all()
    o64.reset_all()
    twin.reset_all()
    drawn = np.unique(o.ep[:, EP["LATENCY"]])
    nominal = perturbed_rows(model, np.tile(identity_record(), (N, 1)), o.ep)
    o.ep[:] = perturbed_rows(model, dynamics_records(N), o.ep)
    rng = np.random.default_rng(0)
    moved = np.zeros(N)
    for t in range(DYN_STEPS):
        act = H.random_actions(model, rng, N)
        ep0, es0, s32, s64, _ = H.oracle_pair_step(o, o64, act, x0)
        twin.ep[:], twin.es[:] = nominal, es0
        xt = x0.copy()
        twin.step(act, xt)
        run = (s64.aux_t[:, L.AUX["DONE"]] == 0) & (xt[:, L.AUX["DONE"]] == 0)
        d = np.abs(s64.es[:, L.ES["QVEL"]:L.ES["QVEL"] + L.NV].astype(np.float64) - twin.es[:, L.ES["QVEL"]:L.ES["QVEL"] + L.NV]).max(1)
        moved = np.where(run, np.maximum(moved, d), moved)
        x0 = s32.aux
    ncase = len(dynamics_cases())
    return {c.name: moved[i::ncase] for i, c in enumerate(dynamics_cases())}, drawn


def dynamics_run(model, make_stepper):
    """The teacher-forced loop of tests/test_gpu_push.py::test_scripted_push_matches_the_oracle under perturbed model rows: DYN_N envs, DYN_STEPS
    steps, seed DYN_SEED, helpers.teacher_forced_config(N, "sampler"), actions helpers.random_actions on default_rng(0); the seven dynamics
    cases and nominal, 8 envs each. `make_stepper(cfg, seed, ep_reset, records) -> (rows, step)`: the implementation under test writes the
    records over the reset rows `ep_reset` ITS way and returns the rows it then holds and `step(ep0, es0, act, aux_in) -> helpers.Step`.
    Both oracles get perturbed_row's rows. Returns (errs, errs_oracle, left_out, rows_got, rows_want): the implementation against the fp32
    oracle and the fp32 oracle against the fp64 one, on the env-steps with DONE == 0, and how many env-steps that left out."""
    from oracle import oracle as Or
    from tests import helpers as H
    N = DYN_N
    cfg = H.teacher_forced_config(N, "sampler")
    o, o64 = Or.Oracle(model, cfg, seed=DYN_SEED, precision="f32"), Or.Oracle(model, cfg, seed=DYN_SEED, precision="f64")
    _, _, x0 = o.reset_all()
    o64.reset_all()
    records = dynamics_records(N)
    want = perturbed_rows(model, records, o.ep)
    got, step = make_stepper(cfg, DYN_SEED, o.ep.copy(), records)
    o.ep[:] = want
    rng = np.random.default_rng(0)
    errs, errs_o, left_out = {k: [] for k in H.TOL}, {k: [] for k in H.TOL}, 0
    for t in range(DYN_STEPS):
        act = H.random_actions(model, rng, N)
        ep0, es0, s32, s64, _ = H.oracle_pair_step(o, o64, act, x0)
        s = step(ep0, es0, act, x0)
        assert np.array_equal(s32.aux_t[:, L.AUX["DONE"]], s.aux_t[:, L.AUX["DONE"]]), f"DONE differs from the oracle's at step {t}"
        run = s32.aux_t[:, L.AUX["DONE"]] == 0
        left_out += int((~run).sum())
        for k, v in H.state_errors(o.es, s.es).items():
            errs[k].append(v[run])
        for k, v in H.state_errors(s64.es, s32.es).items():
            errs_o[k].append(v[run])
        x0 = s32.aux
    return errs, errs_o, left_out, got, want


def quantiles(errs) -> str:
    return "; ".join(f"{k} median {np.median(np.concatenate(v)):.2e} p99 {np.quantile(np.concatenate(v), 0.99):.2e} max {np.concatenate(v).max():.2e}" for k, v in errs.items())
