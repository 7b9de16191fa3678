#!/bin/bash
# A/B runs of bench.py under environment settings (GPU box): tools/ab_env.sh "A=1 B=2" "C=3" ...  -> one summary line per setting
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
for s in "$@"; do
  env $s timeout -k 10 400 python bench.py --full --e2e-reads 0 --cpu-sample 20000 > "$TMP/ab.json" 2> "$TMP/ab.err" || { echo "$s: FAILED"; tail -3 "$TMP/ab.err"; continue; }
  python - "$s" "$TMP/ab.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print("%-40s value %.1f Mreads/s  step %.3f ms  serialized %s  parity %s" % (sys.argv[1] or "defaults", d["value"], d["ms_per_step"], d.get("kernel_ms_serialized"), d["parity"]["mismatching_reads"]))
PY
done
