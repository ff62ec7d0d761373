#!/bin/bash
# A window of every frame of a batch against whole batch decode + crop at 256 x 512^2 (224^2 windows), 64 x 2048^2 and 2 x 8192^2 (512^2 windows)
# on this build, the whole form alone on a build of the parent commit (YK_PARENT_TREE = its checkout, built), and the whole-batch check:
# profiles/decode_batch/batch_vs_loop.py on both builds, alternating, three each -- all in one visit.
# Run from the repository root; every GPU step has its own time limit and the steps are chained: nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_batch_window/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_batch_window/window_vs_whole.py
B=profiles/decode_batch/batch_vs_loop.py
OUT=${1:-profiles/decode_batch_window}
mkdir -p "$OUT"
: > "$OUT/window_vs_whole.txt"
: > "$OUT/whole_batch_ab.txt"
new() { timeout -k 10 "$1" python $S $2 $3 $4 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/window_vs_whole.txt"; }
parent() { [ -z "$YK_PARENT_TREE" ] || YK_TREE=$YK_PARENT_TREE timeout -k 10 "$1" python $S $2 $3 $4 7 --whole-only 2>&1 | grep -v amdgpu.ids | sed 's/^/parent: /' | tee -a "$OUT/window_vs_whole.txt"; }
# the whole-batch path: the parent's own spread against this build's, the same frames and sizes
ab() {
    [ -z "$YK_PARENT_TREE" ] && return 0
    YK_TREE=$YK_PARENT_TREE timeout -k 10 "$1" python $YK_PARENT_TREE/$B $2 $3 7 2>&1 | grep -v amdgpu.ids | grep "batch:" | sed "s/^/parent $4: /" | tee -a "$OUT/whole_batch_ab.txt" &&
    timeout -k 10 "$1" python $B $2 $3 7 2>&1 | grep -v amdgpu.ids | grep "batch:" | sed "s/^/new $4: /" | tee -a "$OUT/whole_batch_ab.txt"
}
new 240 256 512 224 && parent 240 256 512 224 &&
new 300 64 2048 512 && parent 300 64 2048 512 &&
new 300 2 8192 512 && parent 300 2 8192 512 &&
ab 240 256 512 1 && ab 240 256 512 2 && ab 240 256 512 3 &&
ab 300 64 2048 1 && ab 300 64 2048 2 &&
ab 300 2 8192 1 && ab 300 2 8192 2
