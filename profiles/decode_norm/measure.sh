#!/bin/bash
# Normalised, mirrored pixel windows from the de-tile kernel against the uint8 call followed by torch (norm_vs_torch.py): 256 x 512^2 with 224^2
# windows as CHW fp16, 64 x 2048^2 with 512^2 windows as CHW fp16 and HWC fp32, a 512^2 window of an 8192^2 image as CHW fp16; then bench.py
# --stage decode on a build of the parent commit (YK_PARENT_TREE = its checkout, built) and on this build, alternating, three each.
# Run from the repository root; every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_norm/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_norm/norm_vs_torch.py
OUT=${1:-profiles/decode_norm}
mkdir -p "$OUT"
: > "$OUT/norm_vs_torch.txt"
timeout -k 10 240 python $S 256 512 224 float16 chw 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/norm_vs_torch.txt" &&
timeout -k 10 300 python $S 64 2048 512 float16 chw 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/norm_vs_torch.txt" &&
timeout -k 10 300 python $S 64 2048 512 float32 hwc 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/norm_vs_torch.txt" &&
timeout -k 10 240 python $S 1 8192 512 float16 chw 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/norm_vs_torch.txt" || exit 1
if [ -n "$YK_PARENT_TREE" ]; then
    : > "$OUT/bench_ab.txt"
    for i in 1 2 3; do
        for v in parent new; do
            if [ $v = parent ]; then B=$YK_PARENT_TREE/bench.py; else B=bench.py; fi
            timeout -k 10 300 python $B --gpus 1 --stage decode --device-streams --steps 40 --warmup 5 --no-cpu --no-parity 2>&1 | grep -v amdgpu.ids | tail -1 | sed "s/^/$v $i: /" | tee -a "$OUT/bench_ab.txt" || exit 1
        done
    done
fi
