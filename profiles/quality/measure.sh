#!/bin/bash
# Round-trip quality on the device at the three sizes, then ONE rocprofv3 kernel trace at 64 x 2048^2, apart from the timed runs.  Run from the
# repository root; every GPU step has its own time limit and nothing starts after a failure.
#   profiles/quality/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/quality/quality_prof.py
OUT=${1:-profiles/quality}
mkdir -p "$OUT"
: > "$OUT/quality.txt"
for c in "256 512" "64 2048" "1 8192"; do
    timeout -k 10 300 python $S $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/quality.txt" || exit 1
done
T=$(mktemp -d)
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$T" -o quality -- python $S 64 2048 1 --profile > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
find "$T" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_64x2048.csv" \;
rm -rf "$T"
