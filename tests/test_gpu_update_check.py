"""What kbj_ppo_grad runs between the GEMMs and the recurrences, kernel by kernel (tools/update_check.hip, built from source with hipcc on the box
that runs it, like the other kernel checks): the minibatch gathers and re-pitching kernels, the actor head over a minibatch trajectory with its two
time scans, the Gaussian log-prob, the advantage statistics, ppo_loss_kernel with its three part masks and both normalisation branches,
critic_head_kernel<VPL> at all eight hidden sizes, the mirror loss, the metrics line, matvec / matvec_t_acc / outer_acc / colsum and sumsq - the
atomic and the deterministic first stages alike.

The tool launches the kernels through the *_launch helpers kbj_nn.hip itself calls, every array between guard words, outputs prefilled with a
pattern so that an element a launch must leave alone is demanded unchanged. References are double precision from the stored inputs of the stage
under test, bounds are counted roundings, and the links between launches (scan chunking, resets, single rows, part 1 + part 2 == part 3, the
ordered second stages over the device's own partials) are demanded bit for bit. `update_check --plan` (no device, runs in the CPU suite) proves over
the same case table that every branch of the losses is live and no sample sits on a threshold, that the demanded summation orders can be told from
a balanced tree, that the checker passes a host fp32 model of every kernel and that it rejects every mutant of that model wherever a case
exercises the mutated feature."""
import pytest

from tests import check_tool
from tests.check_tool import case_lines as _case_lines
from tests.helpers import HPARAM_CASES, HPARAM_HEAD_CASES

gpu = pytest.mark.gpu      # per test: the --plan test below needs no device

ALL_H = [64, 128, 192, 256, 320, 384, 448, 512]
LOSS_FIELDS = {"clip_param", "value_clip", "value_loss_coef", "entropy_coef", "log_ratio_clip", "adv_eps"}
# the rows of the ABI tests' table that set nothing but fields ppo_loss_kernel reads, and the one that sets everything
LOSS_HP = [n for n, kw in HPARAM_CASES.items() if set(kw) <= LOSS_FIELDS] + ["combined"]

HEAD_MUTS = ["chunk_state_dropped", "keep_of_neighbour_step", "keep_ignored_in_bwd_carry", "alpha_swapped_in_bwd", "cmd_column_off_by_one", "std_from_column_j",
             "clamp_before_var_scale", "clamp_derivative_not_zeroed", "logp_19_joints", "entropy_dropped_from_gs"]
LOSS_MUTS = ["part_mask_ignored", "stats11_ignored", "fp32_branch_at_200", "clip_test_on_d", "value_zero_branch_dropped", "vcoef_dropped", "inv_r_minus_1"]
CRITIC_MUTS = ["value_zero_branch_dropped", "vcoef_dropped", "inv_r_minus_1", "critic_bias_dropped", "critic_dh_neighbour_row", "critic_dout_column_1"]
GATHER_MUTS = ["idx_ignored", "t_stride_b"]
MUTANTS = {"gather_rows": GATHER_MUTS, "gather_rows4": GATHER_MUTS, "gather_small": GATHER_MUTS, "gather_carry": ["idx_ignored"], "mirror_rows": [], "repitch_rows": [],
           "repitch_pad": [], "actor_train": HEAD_MUTS, "adv_stats": [], "sumsq": ["sumsq_without_scale"], "ppo_loss": LOSS_MUTS, "critic_head": CRITIC_MUTS,
           "mirror_loss": ["mirror_map_identity", "mirror_sign", "part_mask_ignored"], "ppo_metrics": [], "matvec": [], "matvec_t_acc": [], "outer_acc": [],
           "colsum": ["colsum_last_phase_dropped", "colsum_ld_as_n"]}


def test_the_loss_rows_of_the_hyperparameter_table():
    assert LOSS_HP == ["entropy_coef=0.5", "value_loss_coef=2", "clip_param=0.05", "clip_param=0.6", "value_clip=0.05", "value_clip=5", "log_ratio_clip=0.25",
                       "adv_eps=0.5", "combined"]


@pytest.fixture(scope="module")
def plan():
    return check_tool.run("update_check", "--plan", timeout=300)


@pytest.fixture(scope="module")
def report():
    return check_tool.run("update_check", timeout=300)


def _expected():
    """(kernel, description, {mutant: exercised}) of every case: the table of the tool's main()."""
    rows = []

    def gather_rows(t, n, b, w, lds, ldd, scalar, repeat=False):
        rows.append(("gather_rows" if scalar else "gather_rows4", f"T={t} N={n} B={b} w={w} lds={lds} ldd={ldd} form={'rows' if scalar else 'rows4'}{' repeat' if repeat else ''}",
                     dict(idx_ignored=True, t_stride_b=t > 1 and b != n)))
    for t in (1, 3):
        for n in (5, 70):
            for b in (1, 5, 33, 64):
                if b <= n:
                    for scalar in (False, True):
                        gather_rows(t, n, b, 68, 68, 68, scalar)
    for w in (72, 476):
        for b in (33, 64):
            for scalar in (False, True):
                gather_rows(3, 70, b, w, w, w, scalar)
    for scalar in (False, True):
        gather_rows(3, 70, 33, 68, 476, 72, scalar)
        gather_rows(3, 70, 33, 68, 68, 68, scalar, repeat=True)
    for t, n, b in ((3, 70, 33), (1, 5, 5)):
        for old in ("given", "null"):
            for c0, c1 in ((24, 25), (0, 24), (0, 25)):
                rows.append(("gather_small", f"T={t} N={n} B={b} cols=[{c0},{c1}) old={old}", dict(idx_ignored=True, t_stride_b=t > 1 and b != n)))
    for planes in (4, 16):
        for lpf in (0, 2):
            for h in (64, 192, 512):
                rows += [("gather_carry", f"planes={planes} lpf={lpf} H={h} B={b} N=70", dict(idx_ignored=True)) for b in (1, 33)]
    for table, ld in (("actor", 68), ("critic", 476)):
        rows += [("mirror_rows", f"table={table} ld={ld} rows={r}", {}) for r in (1, 33)]
    rows += [("repitch_rows", "rows=64 cols=475 ld=476", {}), ("repitch_rows", "rows=3 cols=5 ld=8", {})]
    rows += [("repitch_pad", f"rows=33 ws={ws} wd=68", {}) for ws in (65, 68, 72)]

    def head(t, b, ld, hp, keep, dy=0, dent=1, form="policy", chained=False):
        alpha1 = hp == "lpf_alpha=1"
        rows.append(("actor_train", f"T={t} B={b} ld={ld} hp={hp} keep={keep} dy={dy} dent={dent} form={form}{' chained' if chained else ''}",
                     dict(chunk_state_dropped=t > 10 and not alpha1, keep_of_neighbour_step=keep in ("hashed", "single") and t > 1 and not alpha1,
                          keep_ignored_in_bwd_carry=keep != "none" and t > 1 and not alpha1, alpha_swapped_in_bwd=True, cmd_column_off_by_one=True, std_from_column_j=True,
                          clamp_before_var_scale=True, clamp_derivative_not_zeroed=form != "mirror", logp_19_joints=True, entropy_dropped_from_gs=dent == 1)))
    for t in (1, 9, 10, 11, 19, 20, 21, 30):
        for b in (3, 33):
            head(t, b, 68, "default", "hashed", chained=(t == 21 and b == 33))
    for t in (11, 21):
        for b in (1, 4):
            head(t, b, 68, "default", "hashed")
    head(11, 33, 72, "default", "hashed")
    for hp in HPARAM_HEAD_CASES:
        head(21, 33, 68, hp, "hashed", chained=True)
    for keep in ("none", "all", "single"):
        for t in (11, 21):
            head(t, 33, 68, "default", keep)
    head(11, 33, 68, "default", "hashed", dy=1)
    head(11, 33, 68, "default", "hashed", dent=0)
    for t in (11, 21):
        head(t, 33, 68, "default", "hashed", dy=1, dent=0, form="mirror")

    for form in ("atomic", "part"):
        rows += [("adv_stats", f"R={r} ratio=0 form={form}", {}) for r in (1, 255, 256, 257, 8191, 8192, 8193, 20000)]
    for form in ("atomic", "part"):
        rows += [("adv_stats", f"R=20000 ratio={q} form={form}", {}) for q in (7, 9, 200)]

    def loss(r, part, ratio, stats, pp):
        rows.append(("ppo_loss", f"R={r} part={part} ratio={ratio} stats={stats} pp={pp}",
                     dict(part_mask_ignored=part != 3, stats11_ignored=stats == "foreign" and bool(part & 1), fp32_branch_at_200=ratio == 200 and bool(part & 1) and r > 1,
                          clip_test_on_d=r >= 255 and bool(part & 1), value_zero_branch_dropped=r >= 255 and bool(part & 2), vcoef_dropped=bool(part & 2),
                          inv_r_minus_1=bool(part & 2) or (bool(part & 1) and r > 1))))
    for r in (1, 255, 256, 257, 1000):
        for part in range(4):
            loss(r, part, 0, "own", "default")
    for ratio in (0, 7, 9, 200):
        loss(1000, 3, ratio, "adv_stats", "default")
        loss(1000, 3, ratio, "foreign", "default")
    for pp in LOSS_HP:
        loss(257, 3, 0, "own", pp)
    for h in ALL_H:
        rows += [("critic_head", f"H={h} R={r}", dict(value_zero_branch_dropped=False, vcoef_dropped=True, inv_r_minus_1=True, critic_bias_dropped=True,
                                                       critic_dh_neighbour_row=r > 1, critic_dout_column_1=True)) for r in (1, 3, 4, 5, 100)]
    for h in (64, 512):
        rows += [("critic_head", f"H={h} R={r}", {m: True for m in CRITIC_MUTS}) for r in (8192, 8193, 8200)]
    for r in (1, 257):
        rows += [("mirror_loss", f"R={r} part={part}", dict(mirror_map_identity=bool(part & 1), mirror_sign=bool(part & 1), part_mask_ignored=part != 3)) for part in (1, 2, 3)]
    for r in (1, 1000):
        rows += [("ppo_metrics", f"R={r} stats={k}", {}) for k in ("own", "foreign", "negative_var")]

    rows += [("matvec", f"M={4 * h} K={h} add=1", {}) for h in ALL_H]
    for add in (0, 1):
        rows += [("matvec", f"M=5 K=65 add={add}", {}), ("matvec", f"M=1 K=1 add={add}", {})]
    for form in ("atomic", "part"):
        rows += [("matvec_t_acc", f"K={4 * h} N={h} form={form}", {}) for h in (64, 192, 512)] + [("matvec_t_acc", f"K=7 N=65 form={form}", {})]
    rows += [("outer_acc", "M=256 N=64", {}), ("outer_acc", "M=2048 N=512", {}), ("outer_acc", "M=3 N=5", {})]

    def colsum(m, n, ld, form):
        rows.append(("colsum", f"M={m} N={n} ld={ld} form={form}", dict(colsum_last_phase_dropped=m > 3, colsum_ld_as_n=ld != n and m > 1)))
    for form in ("atomic", "part"):
        for m in (1, 3, 2047, 2048, 2049, 5000):
            colsum(m, 40, 40, form)
        for n in (1, 64, 65, 256):
            colsum(2049, n, n, form)
            colsum(2049, n, n + 3, form)
        colsum(5000, 1, 40, form)
        colsum(3, 40, 43, form)
    for form in ("atomic", "part"):
        rows += [("sumsq", f"n={n} scale=1 form={form}", dict(sumsq_without_scale=False)) for n in (1, 255, 256, 257, 131071, 131072, 131073, 300000)]
    for form in ("atomic", "part"):
        rows += [("sumsq", f"n=131073 scale={s} form={form}", dict(sumsq_without_scale=True)) for s in ("0.125", "1/3")]
    return rows


def _find(lines, kernel, desc):
    hits = [l for l in lines if l.split()[1] == kernel and l.split(" : ")[0].split(None, 2)[2].strip() == desc]
    assert len(hits) == 1, (kernel, desc, hits)
    return hits[0]


def _check_table(so):
    lines, rows = _case_lines(so), _expected()
    for kernel, desc, _ in rows:
        _find(lines, kernel, desc)
    assert len(lines) == len(rows)


def _order_demanded(kernel, desc):
    """Where the tool demands a summation order bit for bit AND the partials are many enough for a balanced tree to differ."""
    if "form=part" not in desc:
        return None
    f = dict(kv.split("=", 1) for kv in desc.split() if "=" in kv)
    if kernel == "adv_stats":
        return int(f["R"]) > 4096
    if kernel == "sumsq":
        return int(f["n"]) > 4096
    if kernel == "matvec_t_acc":
        return int(f["K"]) >= 64
    if kernel == "colsum":
        return int(f["M"]) >= 2047
    return None


def test_plan_inputs_live_orders_distinct_model_accepted_every_mutant_rejected(plan):
    """No device. Every outcome of the policy and the value loss holds >= 5 % of the samples of a case with R >= 255, the std clamp 10 % .. 90 % of
    an actor case's entries, and no sample is within 8 x its fp32 error bound of a threshold (the re-draws are printed); where a summation order
    is demanded a balanced tree gives other bits; the checker passes the host fp32 model of every kernel; every mutant is rejected by more than
    100 x the bound wherever the case exercises the feature, and says n/a exactly where it does not."""
    check_tool.assert_finished(*plan, "UPDATE CHECK PLAN OK")
    so = plan[1]
    _check_table(so)
    lines = _case_lines(so)
    for kernel, desc, exercised in _expected():
        l = _find(lines, kernel, desc)
        assert " planned" in l and " model ok" in l, l
        assert sorted(exercised) == sorted(MUTANTS[kernel]), (kernel, desc)
        for mut, on in exercised.items():
            want = "rejected" if on else "n/a"
            assert f" {mut}={want}" in l, (mut, want, l)
        if kernel in ("ppo_loss", "critic_head", "actor_train"):
            assert int(l.split(" margin_violations ")[1].split()[0]) == 0 and int(l.split(" redraws ")[1].split()[0]) >= 0, l
        if kernel == "actor_train":
            assert 0.1 <= float(l.split(" clamp ")[1].split()[0]) <= 0.9, l
        if kernel in ("ppo_loss", "critic_head") and int(desc.split("R=")[1].split()[0]) >= 255:
            shares = ("in", "zero", "taken", "lr", "vi", "va", "vz") if kernel == "ppo_loss" else ("vi", "va", "vz")
            assert all(float(l.split(f" {s} ")[1].split()[0]) >= 0.05 for s in shares), l
        demanded = _order_demanded(kernel, desc)
        if demanded is not None:
            assert (" order=distinct" if demanded else " order=n/a") in l, l
    for mut in set(sum(MUTANTS.values(), [])):      # every mutant is exercised, and rejected, somewhere
        assert any(f" {mut}=rejected" in l for l in lines), mut


@gpu
def test_every_update_kernel_matches_the_host_reference(report, plan):
    check_tool.assert_finished(*report, "UPDATE CHECK PASSED")
    assert len(_case_lines(report[1])) == len(_case_lines(plan[1]))


@gpu
def test_the_case_table_is_the_one_the_kernels_are_launched_at(report):
    _check_table(report[1])
