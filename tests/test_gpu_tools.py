"""GPU checks that live in stand-alone programs under tools/ (built from source with hipcc on the box that runs them) and belong in the
driver's `-m gpu` run:

* tools/wave_test: every wave primitive of csrc/kbj_wave.h and the whole arrow (LDL^T) solve of the env kernel's register solver on the GPU
  against the host emulation of the SAME source - bit for bit for the primitives; the solve, whose pivots go through v_rcp_f32 on the GPU and
  through a division in the emulation, to 1e-6 of the emulation's and 2e-6 of a double-precision dense solve (measured 2.2e-7 / 4.0e-7).
  This is what lets tests/test_emu_env.py (CPU) speak for the register solver the GPU runs.
* tools/gemm_bench 10: the operand range of the bf16 x3 split GEMM (kbj_config.gemm_bf16x3): as accurate as the exact fp32-MFMA kernel for
  operands scaled anywhere in 2^-100 .. 2^100, bounded loss below 2^-110 where the split's lower pieces enter the bf16 subnormal range.
* tools/gemm_check: every form of the GEMM launcher (csrc/kbj_gemm.h), named after its call site in kbj_nn.hip, against a full double-precision
  reference at ragged shapes inside NaN / bit-pattern guard bands - bit for bit on integer operands, within the derived fp32 bound on reals;
  `gemm_check --plan` (no device, runs in the CPU suite) proves that the integer inputs satisfy the bit-exactness precondition.
"""
import pytest

from tests import check_tool

gpu = pytest.mark.gpu      # per test: the --plan test below needs no device


@gpu
def test_wave_primitives_and_arrow_solve_bit_identical_to_the_emulation():
    rc, so, se = check_tool.run("wave", timeout=300, binary="wave_test/wave_test")
    assert rc == 0 and "WAVE TEST PASSED" in so, (so[-2000:], se[-500:])
    lines = [l for l in so.splitlines() if l.strip()]
    prim = [l for l in lines if l.split()[1:2] == ["ok"]]
    assert len(prim) == 16, so                                   # sixteen primitives, every one reported lane-exact
    assert not any("FAIL" in l for l in lines), so
    solve = [l for l in lines if l.startswith("arrow_solve_w")]
    import re
    m = re.search(r"GPU vs emulation ([0-9.eE+-]+), GPU vs double dense solve ([0-9.eE+-]+)", solve[0]) if solve else None
    assert m and float(m.group(1)) < 1e-6 and float(m.group(2)) < 2e-6, solve     # relative to max |x| over 256 random arrow systems


@gpu
def test_gemm_bf16x3_operand_range():
    rc, so, se = check_tool.run("gemm_bench", "10", timeout=600)
    assert rc == 0 and "X3 RANGE TEST PASSED" in so, (so[-3000:], se[-500:])
    rows = [l for l in so.splitlines() if l.lstrip().startswith("A x 2^")]
    assert len(rows) == 24 and all(l.rstrip().endswith("ok") or "bounded loss" in l for l in rows), so
    strict = [l for l in rows if "bounded loss" not in l]
    assert len(strict) == 16                                       # every operand scale in 2^-100 .. 2^100: as accurate as the exact kernel


GEMM_CHECK_FORMS = ("linear_fwd", "rollout_gates", "critic_input_projection", "g2a", "linear_bwd_input", "linear_bwd_weight", "linear_bwd_weight2",
                    "g1a")


def test_gemm_check_plan_inputs_satisfy_the_exactness_precondition():
    """No device: the tool enumerates its case table, builds the integer inputs and verifies that sum |a||b| + |bias| + |C0| < 2^24 for every
    output element, i.e. that the reference alone entitles the GPU test to demand bit-identical results."""
    rc, so, se = check_tool.run("gemm_check", "--plan", timeout=300)
    check_tool.assert_finished(rc, so, se, "GEMM CHECK PLAN OK")
    cases = check_tool.case_lines(so)
    for form in GEMM_CHECK_FORMS:                                   # every call site of kbj_nn.hip, as issued and with x3 = 1
        mine = [l for l in cases if l.split()[2] == form]
        assert any(" x3=0->" in l for l in mine) and any(" x3=1->" in l for l in mine), form
    x3 = [l for l in cases if " x3=1->" in l]
    for kind in ("x3-plain(TM=1)", "x3-plain(TM=2)", "x3-GEN(TM=1)", "x3-GEN(TM=2)", "exact-kernel("):   # all four instantiations and the fallback
        assert any(kind in l for l in x3), kind


@gpu
def test_gemm_check_every_form_against_the_double_reference():
    rc, so, se = check_tool.run("gemm_check", "--plan", timeout=300)
    check_tool.assert_finished(rc, so, se, "GEMM CHECK PLAN OK")
    planned = len(check_tool.case_lines(so))
    rc, so, se = check_tool.run("gemm_check", timeout=300)
    check_tool.assert_finished(rc, so, se, "GEMM CHECK PASSED")
    cases = check_tool.case_lines(so)
    assert len(cases) == planned, (len(cases), planned)
    for form in GEMM_CHECK_FORMS:
        assert any(l.split()[2] == form for l in cases), form
