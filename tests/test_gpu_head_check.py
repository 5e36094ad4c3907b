"""The kernels behind the last LSTM layer of the rollout on their own (actor_head_fused_kernel, critic_value_fused_kernel, carry_reset_kernel,
lstm_cell_fwd_kernel, actor_head_lpf_kernel, init_uniform_kernel) and every threefry draw of the action and init streams, against a double /
exact host reference (tools/head_check.hip, built from source with hipcc on the box that runs it, like the other kernel checks).

The tool launches the kernels through the launch helpers kbj_nn.hip itself calls. The actor head runs twice per case (argmax, sampled) from the
same inputs; bounds are propagated from the projection's gamma_n, the links (lpf untouched by sampling, mode == lpf, single rows relaunched
alone, the pure-draw log-prob sum, carry reset, init) are demanded bit for bit, and every sampled action is held to z_ref formed from the
exact threefry words. `head_check --plan` (no device, runs in the CPU suite) proves over the same case table that the clamp and both softplus
branches are live, that the host draws are sound, that the checker passes a host fp32 model of every kernel and that it rejects eleven mutants
of that model wherever a case exercises the mutated feature."""
import pytest

from tests import check_tool
from tests.check_tool import case_lines as _case_lines
from tests.helpers import HPARAM_HEAD_CASES

gpu = pytest.mark.gpu      # per test: the --plan test below needs no device

ALL_H = [64, 128, 192, 256, 320, 384, 448, 512]
HEAD_N = [1, 15, 16, 17, 63, 64, 65, 100, 130]
LD = [68, 72]              # layout.obs_widths: 65 columns -> 68, with 4..7 user columns -> 72
OFFS, STEPS = [1000, 0xFFFFFFF0], [5, 0x80000007]

ACTOR_MUTS = ["env_off_ignored", "tile_local_env", "counter_swapped", "u1_without_plus1", "std_from_column_j", "cmd_column_off_by_one",
              "clamp_before_var_scale", "lpf_wrong_operand", "logp_19_joints"]
MUTANTS = {"actor": ACTOR_MUTS, "actor_pure": ACTOR_MUTS, "lpf": ["cmd_column_off_by_one", "lpf_wrong_operand"], "init": ["leaf_ignored"],
           "carry": ["negzero_is_done"], "critic": [], "cell": []}


def test_the_second_row_stride_is_the_next_the_layout_gives():
    from kbot_joystick_amd.spec import layout as L
    widths = sorted({L.ld_of(L.NOBS_ACTOR + k) for k in range(8)})
    assert widths[:2] == LD


@pytest.fixture(scope="module")
def plan():
    return check_tool.run("head_check", "--plan", timeout=300)


@pytest.fixture(scope="module")
def report():
    return check_tool.run("head_check", timeout=300)


def _expected():
    """(kernel, description, traits) of every kernel case: the table of the tool's main()."""
    rows = []

    def actor(h, n, ld, off, step, hp):
        rows.append(("actor", f"H={h} N={n} ld={ld} off={off} step={step} hp={hp}", dict(N=n, off=off)))
    for h in (64, 256):
        for n in HEAD_N:
            actor(h, n, 68, 0, 0, "default")
    for h in ALL_H:
        actor(h, 33, 68, 0, 0, "default")
    for n in (33, 100):
        actor(64, n, 72, 0, 0, "default")
    for off in OFFS:
        for step in STEPS:
            for h in (64, 256):
                actor(h, 100, 68, off, step, "default")
    for hp in HPARAM_HEAD_CASES:
        actor(64, 33, 68, 1000, 5, hp)
    for n, off, step, seed in ((100, 0, 0, "fixed"), (130, 1000, 5, "fixed"), (100, 0xFFFFFFF0, 0x80000007, "fixed"), (130, 1000, 5, "tail")):
        rows.append(("actor_pure", f"H=64 N={n} off={off} step={step} seed={seed}", dict(N=n, off=off, tail=seed == "tail")))
    for n in (1, 7, 8, 9, 100):
        rows += [("critic", f"H={h} N={n}", {}) for h in ALL_H]
    for cnt in (1, 3, 4, 5, 130):
        for h in (64, 192, 512):
            for planes in (2, 8):
                for lpf in (1, 0):
                    for stride in (1, 72):
                        rows += [("carry", f"cnt={cnt} H={h} planes={planes} lpf={lpf} stride={stride} done={d}", dict(hashed=d == "hashed")) for d in ("none", "all", "hashed")]
    for m in (1, 33):
        for h in (64, 256, 512):
            rows += [("cell", f"H={h} M={m} masked={k}", {}) for k in (0, 1)]
    for n in (1, 13, 100):
        rows += [("lpf", f"N={n} ld={ld}", {}) for ld in LD]
    for n in (1, 255, 256, 257, 70001):
        for leaf in (0, 7):
            rows += [("init", f"n={n} leaf={leaf} bound={b}", dict(leaf=leaf)) for b in ("1/8", "1/sqrt(475)")]
    return rows


def _exercised(kernel, mut, t):
    """Does the case exercise what the mutant breaks?"""
    return {"env_off_ignored": t.get("off", 0) != 0, "tile_local_env": t.get("N", 0) > 16, "u1_without_plus1": t.get("tail", False),
            "lpf_wrong_operand": kernel != "actor_pure", "leaf_ignored": t.get("leaf", 0) != 0, "negzero_is_done": t.get("hashed", False)}.get(mut, True)


def _find(lines, kernel, desc):
    hits = [l for l in lines if l.split()[1] == kernel and l.split(" : ")[0].split(None, 2)[2].strip() == desc]
    assert len(hits) == 1, (kernel, desc, hits)
    return hits[0]


def _check_table(so):
    lines, rows = _case_lines(so), _expected()
    for kernel, desc, _ in rows:
        _find(lines, kernel, desc)
    assert len([l for l in lines if l.split()[1] == "draws"]) == 1
    assert len(lines) == len(rows) + 1


def test_plan_inputs_live_draws_sound_model_accepted_every_mutant_rejected(plan):
    """No device. The clamp holds 10 % .. 90 % of every actor case's std entries and both softplus branches are reached; the host draws over
    2^20+ triples pass their five tests at 5 sigma; the checker passes the host fp32 model of every kernel; every mutant is rejected by more
    than 100 x the bound wherever the case exercises the feature, and says n/a exactly where it does not."""
    check_tool.assert_finished(*plan, "HEAD CHECK PLAN OK")
    so = plan[1]
    _check_table(so)
    lines = _case_lines(so)
    for kernel, desc, traits in _expected():
        l = _find(lines, kernel, desc)
        assert " planned" in l and " model ok" in l, l
        if kernel == "actor":
            assert 0.1 <= float(l.split(" clamp ")[1].split()[0]) <= 0.9, l
            assert int(l.split(" sp_hi ")[1].split()[0]) > 0 and int(l.split(" sp_lo ")[1].split()[0]) > 0, l
        for mut in MUTANTS[kernel]:
            want = "rejected" if _exercised(kernel, mut, traits) else "n/a"
            assert f" {mut}={want}" in l, (mut, want, l)
    draws = [l for l in lines if l.split()[1] == "draws"][0]
    assert float(draws.split(" triples ")[1].split()[0]) >= 2 ** 20
    sigmas = [float(draws.split(f" {k} ")[1].split()[0]) for k in ("mean", "var", "rho_env", "rho_step", "rho_joint")]
    assert all(abs(s) < 5 for s in sigmas), draws
    for mut in set(sum(MUTANTS.values(), [])):      # every mutant is exercised, and rejected, somewhere
        assert any(f" {mut}=rejected" in l for l in lines), mut


@gpu
def test_every_head_kernel_and_every_draw_matches_the_host_reference(report, plan):
    check_tool.assert_finished(*report, "HEAD CHECK PASSED")
    assert len(_case_lines(report[1])) == len(_case_lines(plan[1]))


@gpu
def test_the_case_table_is_the_one_the_kernels_are_launched_at(report):
    _check_table(report[1])
