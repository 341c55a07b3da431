#!/bin/bash
# rocprofv3 kernel statistics of bench.py with the given flags:  gpurun -- bash tools/prof_bench.sh <tag> [bench flags]
export TMPDIR=/tmp
tag=$1; shift
ROOT=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)   # the repository (this script lives in tools/)
OUT=${PROF_OUT:-/tmp/prof_bench}; mkdir -p $OUT            # kernel statistics + bench line: $OUT/prof_<tag>/, $OUT/prof_<tag>.log
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$tag -o b -- python $ROOT/bench.py --full --no-cpu-baseline --no-gpu-baseline --no-secondary --steps 30 "$@" > $OUT/prof_$tag.log 2>&1)
tail -1 $OUT/prof_$tag.log | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value']/1e6, d['ms_per_step'], d['roofline']['phases_ms'])"
python - "$OUT/prof_$tag" <<'PY'
import csv, sys
for r in csv.DictReader(open(f"{sys.argv[1]}/b_kernel_stats.csv")):
    if float(r["Percentage"]) > 0.3: print("   ", r["Name"].replace("void ", "").replace("voxe::", "")[:60].ljust(60), r["Calls"], round(float(r["AverageNs"]) / 1e3, 1), r["Percentage"])
PY
