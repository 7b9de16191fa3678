#!/bin/bash
# A/B runs of bench.py under extra arguments (GPU box): tools/ab_args.sh "--streams 6" "--streams 8 --batches 16" ...
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
for s in "$@"; do
  timeout -k 10 400 python bench.py --full --e2e-reads 0 --cpu-sample 20000 $s > "$TMP/ab.json" 2> "$TMP/ab.err" || { echo "$s: FAILED"; tail -3 "$TMP/ab.err"; continue; }
  python - "$s" "$TMP/ab.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print("%-40s value %.1f Mreads/s  step %.3f ms  parity %s" % (sys.argv[1] or "defaults", d["value"], d["ms_per_step"], d["parity"]["mismatching_reads"]))
PY
done
