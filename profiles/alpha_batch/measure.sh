#!/bin/bash
# Batch against loop at the three sizes on this build, then the loops alone on a build of the parent commit (YK_PARENT_TREE = its checkout, built),
# all in one visit; last, ONE rocprofv3 kernel trace of the batch forms at 64 x 2048^2, apart from the timed runs.  Run from the repository root;
# every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/alpha_batch/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/alpha_batch/batch_vs_loop.py
OUT=${1:-profiles/alpha_batch}
mkdir -p "$OUT"
: > "$OUT/batch_vs_loop.txt"
for c in "256 512" "64 2048" "2 8192"; do
    timeout -k 10 200 python $S $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_loop.txt" || exit 1
done
if [ -n "$YK_PARENT_TREE" ]; then
    : > "$OUT/loop_parent.txt"
    for c in "256 512" "64 2048" "2 8192"; do
        YK_TREE=$YK_PARENT_TREE timeout -k 10 200 python $S $c 7 --loop-only 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/loop_parent.txt" || exit 1
    done
fi
T=$(mktemp -d)
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$T" -o alpha_batch -- python $S 64 2048 1 --profile > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
find "$T" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_64x2048.csv" \;
rm -rf "$T"
