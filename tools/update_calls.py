"""Host-order call list of a process from a rocprofv3 --kernel-trace --hip-trace run (no counters in that run): the HIP runtime calls by name,
then every kernel launch with its grid and its stream (queue where the trace has no stream), streams relabelled by first appearance. Two
builds that issue the same schedule print the same list: `cmp` it between them before and after a change to the host code of the update or of
the rollout (the tool reads whatever the traced process called).
usage (GPU box): rocprofv3 --kernel-trace --hip-trace -d <dir> -o run -- python3 <driver>; python3 tools/update_calls.py <dir>/run_results.db
drivers: tools/bench_ppo.py for the update; for the rollout tools/bench_policy.py (kbj_policy_step) or a few lines that call kbj_policy_step,
kbj_carry_reset, kbj_critic_value and kbj_rollout once each on a small context (EXPERIMENTS.md "Rollout schedule refactor" lists the calls)."""
import re
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
for (name,) in db.execute("select name from regions where category like 'HIP_RUNTIME%' order by start, id"):
    print("api", name)
labels = {}
for name, gx, gy, gz, stream, queue in db.execute("select name,grid_x,grid_y,grid_z,stream_id,queue_id from kernels order by corr_id, dispatch_id"):
    lane = ("s", stream) if stream else ("q", queue)
    n = re.sub(r"\(.*", "", name.replace("kbj::", "").replace("(anonymous namespace)::", "").replace("void ", ""))
    print("kernel", n, f"{gx}x{gy}x{gz}", f"lane{labels.setdefault(lane, len(labels))}")
