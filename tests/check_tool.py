"""What the drivers of the stand-alone programs under tools/ share (test_gpu_tools.py, test_gpu_det_reductions.py, test_gpu_lstm_check.py,
test_gpu_head_check.py, test_gpu_update_check.py):
build the program from source with hipcc on the box that runs it, run it, and the closing checks every kernel check's report has to meet."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def run(name, *args, timeout, binary=None):
    """`make -C tools -s <name>`, then the program (tools/<name> unless `binary` names another path under tools/): (rc, stdout, stderr)."""
    out = subprocess.run(["make", "-C", TOOLS, "-s", name], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-1500:])
    out = subprocess.run([os.path.join(TOOLS, binary or name), *args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    print(out.stdout[-6000:])
    return out.returncode, out.stdout, out.stderr


def case_lines(stdout):
    return [l for l in stdout.splitlines() if l.startswith("case ")]


def assert_finished(rc, stdout, stderr, banner):
    """Exit status 0, the closing banner, no FAIL anywhere, and exactly one `cases N` line whose N is the number of `case` lines."""
    failing = [l for l in stdout.splitlines() if "FAIL" in l]
    assert rc == 0 and banner in stdout and not failing, (failing[:40], stdout[-2000:], stderr[-500:])
    count = [l for l in stdout.splitlines() if l.startswith("cases ")]
    assert len(count) == 1 and int(count[0].split()[1]) == len(case_lines(stdout)) > 0
