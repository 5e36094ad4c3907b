"""Every LSTM recurrence kernel on its own (lstm_seq_fwd_kernel in its three forms, lstm_seq_bwd_kernel, lstm_seq_bwd_wide_kernel,
lstm_seq_bwd16_kernel, lstm_step_kernel), step by step against a double-precision reference (tools/lstm_check.hip, built from source with
hipcc on the box that runs it, like tools/gemm_check and tools/reduce_check).

The tool launches the kernels through the launch helpers kbj_nn.hip itself calls. Each step is compared with a double reference of that
step computed from the kernel's own stored inputs, the links between steps (Hout = o TanhC, Hm = Hout keep, slot 0, the deterministic bias
partials) bit for bit: nothing compounds over t, the bounds stay near 1e-6 and one wrong row, unit, gate, step or keep flag is O(1).
`lstm_check --plan` (no device, runs in the CPU suite) proves over the same case table that the gates are not saturated, that the checker
passes a host fp32 model of every kernel and that it rejects eight mutants of that model wherever a case exercises the mutated feature."""
import pytest

from tests import check_tool
from tests.check_tool import case_lines as _case_lines

gpu = pytest.mark.gpu      # per test: the --plan test below needs no device

KEEPS = ["ones", "zeros", "t0", "tlast", "hashed"]          # every recurrence case with T >= 2; T = 1: ones and zeros (the other three coincide with zeros)
ALL_H = [64, 128, 192, 256, 320, 384, 448, 512]
FUSED_H = [64, 128, 192, 256]

# (H, B, T) per kernel: the table of the tool's main()
FWD_PLAIN = ([(h, 33, 3) for h in ALL_H] + [(h, b, t) for h in (64, 256) for b in (1, 32, 70) for t in (1, 2, 5)]
             + [(64, 128, 3), (192, 100, 3)])                                                   # nblk % 8 == 0: the remapped grid
FWD_FUSED = [(h, 33, t) for h in FUSED_H for t in (1, 3)] + [(h, b, t) for h in (64, 256) for b in (1, 70) for t in (1, 3)]
FWD_OBS = [(h, 33, 3, kx) for h in FUSED_H for kx in (65, 68)]
BWD32 = [(h, 33, t) for h in ALL_H for t in (1, 2, 5)] + [(h, b, t) for h in (64, 256, 512) for b in (1, 70) for t in (1, 2, 5)]
BWD16 = [(h, b, t) for h in FUSED_H for b in (1, 15, 16, 17, 48) for t in (1, 2, 5)] + [(64, 128, 2), (256, 32, 2)]
STEP = [(h, m, obs) for h in FUSED_H for obs in (False, True) for m in (1, 33)] + [(256, 1061, False), (64, 4129, False)]


@pytest.fixture(scope="module")
def plan():
    return check_tool.run("lstm_check", "--plan", timeout=300)


@pytest.fixture(scope="module")
def report():
    return check_tool.run("lstm_check", timeout=300)


def _expected():
    """(kernel, description, family, T, keep, B, kx short, bias partials) of every case."""
    rows = []

    def keeps(t):
        return KEEPS if t >= 2 else KEEPS[:2]
    for h, b, t in FWD_PLAIN:
        rows += [("fwd_plain", f"H={h} B={b} T={t} keep={k}", "fwd", t, k, b, False, False) for k in keeps(t)]
    for h, b, t in FWD_FUSED:
        rows += [("fwd_fused", f"H={h} B={b} T={t} keep={k}", "fwd", t, k, b, False, False) for k in keeps(t)]
    for h, b, t, kx in FWD_OBS:
        rows += [("fwd_obs", f"H={h} B={b} T={t} kx={kx} keep={k}", "fwd", t, k, b, kx < 68, False) for k in keeps(t)]
    for table, name16 in ((BWD32, None), (BWD16, "bwd16")):
        for h, b, t in table:
            kernel = name16 or ("bwd" if h <= 256 else "bwd_wide")
            for part in (False, True):
                rows += [(kernel, f"H={h} B={b} T={t} bias={'part' if part else 'atomic'} keep={k}", "bwd", t, k, b, False, part) for k in keeps(t)]
    for h, m, obs in STEP:
        nug, nrg = h // 32, (m + 31) // 32
        grid = nug * max(1, min(nrg, 256 // nug))
        rows.append(("step_obs" if obs else "step", f"H={h} M={m} {'kx=65 ' if obs else ''}grid={grid}", "step", 1, "ones", m, obs, False))
    return rows


def _exercised(fam, mut, t, keep, b, kx_short, part):
    """Does the case exercise what the mutant breaks? (the hashed pattern pins keep[0][0] = 0 and keep[1][0] = 1)"""
    differs_in_t = t >= 2 and keep in ("t0", "tlast", "hashed")
    zero_before_last = t >= 2 and keep in ("zeros", "t0", "hashed")     # BPTT has nothing recurrent to mask at the last step
    return {"keep_ignored": keep != "ones" if fam == "fwd" else zero_before_last, "keep_neighbour": differs_in_t, "cm_unmasked": keep != "ones",
            "kx_beyond": kx_short, "dc_keep_next": differs_in_t, "dh_unmasked": zero_before_last, "cprev_next": True,
            "dbpart_pairwise": part and b >= 3}[mut]


MUTANTS = {"fwd": ["keep_ignored", "keep_neighbour", "cm_unmasked", "kx_beyond"],
           "bwd": ["keep_ignored", "keep_neighbour", "dc_keep_next", "dh_unmasked", "cprev_next", "dbpart_pairwise"],
           "step": ["kx_beyond"]}


def _find(lines, kernel, desc):
    hits = [l for l in lines if l.split()[1] == kernel and l.split(":")[0].split(None, 2)[2].strip() == desc]
    assert len(hits) == 1, (kernel, desc, hits)
    return hits[0]


def _check_table(so):
    lines, rows = _case_lines(so), _expected()
    for kernel, desc, *_ in rows:
        _find(lines, kernel, desc)
    assert len(lines) == len(rows)
    # the step kernel walks several row groups per workgroup: 34 row groups on 32 chunks, 130 on 128
    assert "H=256 M=1061 grid=256" in so and "H=64 M=4129 grid=256" in so


def test_plan_gates_alive_model_accepted_every_mutant_rejected(plan):
    """No device. Per case: >= 90 % of the gate pre-activations within |x| <= 3; the checker passes the host fp32 model; every mutant is
    rejected by more than 100 x the bound wherever the case exercises the feature, and says n/a exactly where it does not."""
    check_tool.assert_finished(*plan, "LSTM CHECK PLAN OK")
    so = plan[1]
    _check_table(so)
    lines = _case_lines(so)
    for kernel, desc, fam, t, keep, b, kx_short, part in _expected():
        l = _find(lines, kernel, desc)
        assert " planned alive " in l and " model ok" in l, l
        assert float(l.split(" alive ")[1].split()[0]) >= 0.9, l
        for mut in MUTANTS[fam]:
            want = "rejected" if _exercised(fam, mut, t, keep, b, kx_short, part) else "n/a"
            assert f" {mut}={want}" in l, (mut, want, l)
    # every mutant is exercised, and rejected, somewhere
    for mut in set(sum(MUTANTS.values(), [])):
        assert any(f" {mut}=rejected" in l for l in lines), mut


@gpu
def test_every_recurrence_kernel_matches_the_stepwise_double_reference(report, plan):
    check_tool.assert_finished(*report, "LSTM CHECK PASSED")
    assert len(_case_lines(report[1])) == len(_case_lines(plan[1]))


@gpu
def test_the_case_table_is_the_one_the_kernels_are_launched_at(report):
    _check_table(report[1])
