#!/bin/bash
# Batch against per-frame stream building at the three sizes on this build, then decode_batch_from_encoder end to end on a build of the parent
# commit (YK_PARENT_TREE = its checkout, built) and on this build, all in one visit.  Run from the repository root; every GPU step has its own
# time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/encode_streams_batch/measure.sh [output directory, default: next to this script]
set -o pipefail
D=profiles/encode_streams_batch
OUT=${1:-$D}
mkdir -p "$OUT"
: > "$OUT/batch_vs_per_frame.txt"; : > "$OUT/e2e_new.txt"
for c in "256 512" "64 2048" "2 8192"; do
    timeout -k 10 240 python $D/batch_vs_per_frame.py $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_per_frame.txt" || exit 1
done
if [ -n "$YK_PARENT_TREE" ]; then
    : > "$OUT/e2e_parent.txt"
    for c in "256 512" "64 2048" "2 8192"; do
        YK_TREE=$YK_PARENT_TREE timeout -k 10 240 python $D/e2e.py $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/e2e_parent.txt" || exit 1
    done
fi
for c in "256 512" "64 2048" "2 8192"; do
    timeout -k 10 240 python $D/e2e.py $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/e2e_new.txt" || exit 1
done
