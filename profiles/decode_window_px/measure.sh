#!/bin/bash
# A window at a pixel offset, cropped in the de-tile, against decoding its aligned cover and slicing it in torch (px_vs_cover.py): a 512^2 window of
# an 8192^2 image, 64 x 2048^2 with 512^2 windows and 256 x 512^2 with 224^2 windows, every origin at (+3, +5) from an aligned one; then bench.py
# --stage decode on a build of the parent commit (YK_PARENT_TREE = its checkout, built) and on this build, alternating, three each.
# Run from the repository root; every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_window_px/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_window_px/px_vs_cover.py
OUT=${1:-profiles/decode_window_px}
mkdir -p "$OUT"
: > "$OUT/px_vs_cover.txt"
timeout -k 10 240 python $S 1 8192 512 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/px_vs_cover.txt" &&
timeout -k 10 300 python $S 64 2048 512 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/px_vs_cover.txt" &&
timeout -k 10 240 python $S 256 512 224 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/px_vs_cover.txt" || exit 1
if [ -n "$YK_PARENT_TREE" ]; then
    : > "$OUT/bench_ab.txt"
    for i in 1 2 3; do
        for v in parent new; do
            if [ $v = parent ]; then B=$YK_PARENT_TREE/bench.py; else B=bench.py; fi
            timeout -k 10 300 python $B --gpus 1 --stage decode --device-streams --steps 40 --warmup 5 --no-cpu --no-parity 2>&1 | grep -v amdgpu.ids | tail -1 | sed "s/^/$v $i: /" | tee -a "$OUT/bench_ab.txt" || exit 1
        done
    done
fi
