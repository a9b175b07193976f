#!/bin/bash
# A/B of the C3 bench against a previous build kept in ab_old/ (a copy of the package, bench.py and
# oracle at that commit, library built there): new, old, new, old, each under its own time limit.
# Both run with --full (the fields compared below are measured only there), so the copy in ab_old/
# must be of a commit whose bench.py has that option.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
out=${L3_OUT_DIR:-bench_out}  # logs go here (default: bench_out/ in the repository root)
mkdir -p "$out"
for i in 1 2; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline > $out/abb_new_$i.log 2>&1 || exit $?
  timeout -k 10 300 python ab_old/bench.py --full --no-cpu-baseline > $out/abb_old_$i.log 2>&1 || exit $?
done
for f in $out/abb_*.log; do
  python - "$f" <<'PY'
import json, sys
l = [x for x in open(sys.argv[1]) if x.startswith("{")][-1]
d = json.loads(l)
print(sys.argv[1], d["ms_per_step"], d["ms_per_step_all_rows_last_layer"], d["ms_per_step_serialized"], d.get("kernel_ms"))
PY
done
