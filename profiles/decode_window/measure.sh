#!/bin/bash
# Window decode against whole decode + crop at 8192 and 16384 on this build, the whole form alone on a build of the parent commit
# (YK_PARENT_TREE = its checkout, built), and bench.py --stage decode on both builds, alternating, five each: all in one visit.
# Run from the repository root; every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_window/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_window/window_vs_whole.py
OUT=${1:-profiles/decode_window}
mkdir -p "$OUT"
: > "$OUT/window_vs_whole.txt"
for size in 8192 16384; do
    timeout -k 10 240 python $S $size 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/window_vs_whole.txt" || exit 1
    if [ -n "$YK_PARENT_TREE" ]; then
        YK_TREE=$YK_PARENT_TREE timeout -k 10 240 python $S $size 7 --whole-only 2>&1 | grep -v amdgpu.ids | sed 's/^/parent: /' | tee -a "$OUT/window_vs_whole.txt" || exit 1
    fi
done
if [ -n "$YK_PARENT_TREE" ]; then
    : > "$OUT/bench_decode_ab.txt"
    for i in 1 2 3 4 5; do
        for v in parent new; do
            if [ $v = parent ]; then B=$YK_PARENT_TREE/bench.py; else B=bench.py; fi
            timeout -k 10 300 python $B --gpus 1 --stage decode --device-streams --steps 40 --warmup 5 --no-cpu --no-parity 2>&1 | grep -v amdgpu.ids | tail -1 | sed "s/^/$v $i: /" | tee -a "$OUT/bench_decode_ab.txt" || exit 1
        done
    done
fi
