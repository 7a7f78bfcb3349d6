#!/bin/bash
# Kernel list of the deflation seed: rocprofv3 --kernel-trace --stats (a run of its own, no
# counters) of `python tools/bench_initializer.py --trace`.  Run from the repository root; the
# summary goes to $1 (default profiles/r07_initializer_kernel_stats.txt).
set -o pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-$root/profiles/r07_initializer_kernel_stats.txt}
tmp=$(mktemp -d)
cd "$tmp" || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$tmp/p" -o p -- \
  python "$root/tools/bench_initializer.py" --trace > "$tmp/log" 2>&1 || { tail -20 "$tmp/log"; exit 1; }
f=$(find "$tmp/p" -name "*kernel_stats.csv" | head -1)
{
  echo "# rocprofv3 --kernel-trace --stats of: python tools/bench_initializer.py --trace"
  echo "# (one utterance; (513,500,8,3) and (257,800,6,3); permutation_free True and False; 6 calls each)"
  echo "# name | calls | avg_us | min_us | max_us | pct"
  python - "$f" <<PY
import csv,sys
for r in list(csv.DictReader(open(sys.argv[1])))[:12]:
    print(r["Name"][:110], "|", r["Calls"], "| %.1f | %.1f | %.1f |"%(float(r["AverageNs"])/1e3,float(r["MinNs"])/1e3,float(r["MaxNs"])/1e3), r["Percentage"])
PY
} > "$out"
cat "$out"
rm -rf "$tmp"
