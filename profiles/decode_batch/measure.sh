#!/bin/bash
# Batch against loop at the three sizes on this build, then the loop alone on a build of the parent commit (YK_PARENT_TREE = its checkout, built)
# and on this build, all in one visit.  Run from the repository root; every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_batch/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_batch/batch_vs_loop.py
OUT=${1:-profiles/decode_batch}
mkdir -p "$OUT"
: > "$OUT/batch_vs_loop.txt"; : > "$OUT/loop_new.txt"
for c in "256 512" "64 2048" "2 8192"; do
    timeout -k 10 240 python $S $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_loop.txt" || exit 1
done
if [ -n "$YK_PARENT_TREE" ]; then
    : > "$OUT/loop_parent.txt"
    for c in "256 512" "64 2048" "2 8192"; do
        YK_TREE=$YK_PARENT_TREE timeout -k 10 240 python $S $c 7 --loop-only 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/loop_parent.txt" || exit 1
    done
fi
for c in "256 512" "64 2048" "2 8192"; do
    timeout -k 10 240 python $S $c 7 --loop-only 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/loop_new.txt" || exit 1
done
