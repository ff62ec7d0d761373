#!/bin/bash
# Reduced-resolution outputs against whole decode + full-size output + a reduction in torch (scaled_vs_full.py): levels 1..3 at 8192 and 16384 and
# for a batch of 256 x 512 x 512; then bench.py --stage decode on a build of the parent commit (YK_PARENT_TREE = its checkout, built) and on this
# build, alternating, five each.  Run from the repository root; every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_scaled/measure.sh [output directory, default: next to this script]
#   YK_SKIP_SCALED=1 runs the bench comparison alone
set -o pipefail
S=profiles/decode_scaled/scaled_vs_full.py
OUT=${1:-profiles/decode_scaled}
mkdir -p "$OUT"
if [ -z "$YK_SKIP_SCALED" ]; then
    : > "$OUT/scaled_vs_full.txt"
    timeout -k 10 240 python $S image 8192 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/scaled_vs_full.txt" &&
    timeout -k 10 300 python $S image 16384 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/scaled_vs_full.txt" &&
    timeout -k 10 240 python $S batch 256 512 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/scaled_vs_full.txt" || exit 1
fi
if [ -n "$YK_PARENT_TREE" ]; then
    : > "$OUT/bench_ab.txt"
    for i in 1 2 3 4 5; do
        for v in parent new; do
            if [ $v = parent ]; then B=$YK_PARENT_TREE/bench.py; else B=bench.py; fi
            timeout -k 10 300 python $B --gpus 1 --stage decode --device-streams --steps 40 --warmup 5 --no-cpu --no-parity 2>&1 | grep -v amdgpu.ids | tail -1 | sed "s/^/$v $i: /" | tee -a "$OUT/bench_ab.txt" || exit 1
        done
    done
fi
