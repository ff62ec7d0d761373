#!/bin/bash
# The decode of N equally shaped frames, loop and batch form (profiles/decode_batch/batch_vs_loop.py, unmodified), on a build of the parent commit
# (YK_PARENT_TREE = its checkout, built) and on this build: at each of the three sizes parent, new, parent, new, all in one visit, so that the two
# parent medians of a size show the spread of one code on this machine.  Then ONE rocprofv3 kernel trace of 2 x 8192^2 per build, apart from the
# timed runs.  Run from the repository root after the build; every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_plan/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_batch/batch_vs_loop.py
OUT=${1:-profiles/decode_plan}
[ -n "$YK_PARENT_TREE" ] || { echo "YK_PARENT_TREE is not set"; exit 1; }
mkdir -p "$OUT"
: > "$OUT/ab.txt"
for c in "256 512" "64 2048" "2 8192"; do
    for round in 1 2; do
        YK_TREE=$YK_PARENT_TREE timeout -k 10 240 python $S $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/ab.txt" || exit 1
        timeout -k 10 240 python $S $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/ab.txt" || exit 1
    done
done
T=$(mktemp -d)
YK_TREE=$YK_PARENT_TREE timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$T/parent" -o decode_plan -- python $S 2 8192 1 > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
find "$T/parent" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_parent.csv" \;
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$T/new" -o decode_plan -- python $S 2 8192 1 > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
find "$T/new" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_new.csv" \;
rm -rf "$T"
