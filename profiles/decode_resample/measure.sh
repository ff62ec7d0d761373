#!/bin/bash
# Per-frame rectangles resampled by the decoder against whole decode + torch's per-frame loop (resample_vs_torch.py): 256 x 512^2 -> 224^2 and
# 64 x 2048^2 -> 512^2 with random resized crops, one 8192^2 image whole -> 1024^2, and the identity-size call against image_norm_batch_device with
# pixel windows; then bench.py --stage decode on a build of the parent commit (YK_PARENT_TREE = its checkout, built) and on this build, alternating,
# three each.  Run from the repository root; every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_resample/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_resample/resample_vs_torch.py
OUT=${1:-profiles/decode_resample}
mkdir -p "$OUT"
: > "$OUT/resample_vs_torch.txt"
timeout -k 10 240 python $S 256 512 224 float16 crop 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/resample_vs_torch.txt" &&
timeout -k 10 300 python $S 64 2048 512 float16 crop 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/resample_vs_torch.txt" &&
timeout -k 10 240 python $S 1 8192 1024 float16 whole 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/resample_vs_torch.txt" &&
timeout -k 10 240 python $S 256 512 224 float16 identity 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/resample_vs_torch.txt" &&
timeout -k 10 300 python $S 64 2048 512 float16 identity 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/resample_vs_torch.txt" || exit 1
if [ -n "$YK_PARENT_TREE" ]; then
    : > "$OUT/bench_ab.txt"
    for i in 1 2 3; do
        for v in parent new; do
            if [ $v = parent ]; then B=$YK_PARENT_TREE/bench.py; else B=bench.py; fi
            timeout -k 10 300 python $B --gpus 1 --stage decode --device-streams --steps 40 --warmup 5 --no-cpu --no-parity 2>&1 | grep -v amdgpu.ids | tail -1 | sed "s/^/$v $i: /" | tee -a "$OUT/bench_ab.txt" || exit 1
        done
    done
fi
