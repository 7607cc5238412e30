#!/bin/bash
# Needs the GPU: one rocprofv3 --pmc pass of any python tool, kernel trace only beside it (counters are collected in a run of their own); prints the
# counters' means per kernel and dispatch.
# The run is ended after PMC_TIMEOUT seconds (600).
# usage: bash tools/pmc_any.sh <tag> "<COUNTER [COUNTER ...]>" <script.py> [args...]
set -u
TAG=$1; shift
PMC=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d "${TMPDIR:-/tmp}/pmc_$TAG.XXXXXX")
cd "$OUT"
S=$1; shift
timeout -k 10 ${PMC_TIMEOUT:-600} rocprofv3 --pmc $PMC --kernel-trace --output-format csv -d "$OUT" -- python3 "$R/$S" "$@" > "$OUT/out.json" 2> "$OUT/err.txt" || { echo "$TAG failed"; exit 1; }
python3 - "$OUT" "$TAG" <<'PY'
import collections, csv, glob, re, sys
acc = collections.defaultdict(list)
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = re.sub(r"\(.*$", "", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", ""))
        if "rocclr" not in name:
            acc[(name, r["Counter_Name"])].append(float(r["Counter_Value"]))
print(sys.argv[2], "|", "; ".join(f"{n} {c} {sum(v) / len(v):.1f} x{len(v)}" for (n, c), v in acc.items()))
PY
