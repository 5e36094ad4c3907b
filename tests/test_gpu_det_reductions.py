"""The ordered second stages of the deterministic update (kbj_config.deterministic): reduce_rows_kernel, reduce_double_kernel and
splitk_reduce_kernel on synthetic partials, bit for bit against the sequential host sum in each kernel's documented order
(tools/reduce_check.hip, built from source with hipcc on the box that runs it, like tools/gemm_check).

The kernels fetch their partials in batches; the ORDER of the additions is the result. The tool's inputs span 2^-20 .. 2^20 with mixed signs
and a non-zero initial output, and before each launch it proves on the host that a pairwise-order sum of the same input differs from the
chain, so a kernel that adds in another order cannot pass. `reduce_check --plan` (no device, runs in the CPU suite) does that host-side proof
alone over the same case table."""
import pytest

from tests import check_tool

gpu = pytest.mark.gpu      # per test: the --plan test below needs no device

REDUCE_ROWS = [(1, 1), (16, 256), (32, 1024), (33, 257), (512, 1), (512, 40), (511, 65)]       # (nparts, n)
REDUCE_DOUBLE = [(1, 1), (32, 2), (512, 1), (513, 3), (7, 64)]                                  # (nblocks, w)


@pytest.fixture(scope="module")
def report():
    return check_tool.run("reduce_check", timeout=120)


def _cases(so, kernel):
    return [l for l in check_tool.case_lines(so) if l.split()[1] == kernel]


def _check_table(so):
    rows, dbl, sk = _cases(so, "reduce_rows"), _cases(so, "reduce_double"), _cases(so, "splitk_reduce")
    for p, n in REDUCE_ROWS:
        assert any(f"partials {p} x {n} " in l for l in rows), (p, n)
    for b, w in REDUCE_DOUBLE:
        assert any(f"partials {b} x {w} " in l for l in dbl), (b, w)
    for m, n in ((70, 130), (128, 256)):
        for s in (2, 24):
            assert any(f" {m} x {n} K={96 * s} sk={s} ({s} written)" in l for l in sk), (m, n, s)
    assert any("sk=24 (4 written)" in l for l in sk)                 # trailing slices empty: skipped as the GEMM skips them
    assert any("paired" in l and "sk=24" in l for l in sk)           # n1 and C2
    # wherever three or more partials are added, the input was proven to tell a tree from the chain
    for l in rows + dbl + sk:
        few = "partials 1 x" in l or "(2 written)" in l
        assert ("order matters" in l) != few, l


def test_plan_every_input_tells_a_pairwise_sum_from_the_chain():
    """No device: the tool builds every case's input and verifies on the host that the pairwise-order sum differs from the sequential one in
    at least one output, i.e. that the GPU test's bit-for-bit demand cannot be met by a kernel that adds in tree order."""
    rc, so, se = check_tool.run("reduce_check", "--plan", timeout=120)
    check_tool.assert_finished(rc, so, se, "REDUCE CHECK PLAN OK")
    _check_table(so)


@gpu
def test_every_second_stage_is_bit_identical_to_the_sequential_sum(report):
    check_tool.assert_finished(*report, "REDUCE CHECK PASSED")


@gpu
def test_the_case_table_is_the_one_the_kernels_are_launched_at(report):
    _check_table(report[1])
