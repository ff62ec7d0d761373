#!/bin/bash
# encode_files_device against the loop of batch-of-one calls at the three sizes and ZStd levels 3 and 0, convert_bench (ConvertHotPath, level 18 only;
# it draws the YAIK-synth v1 frames itself, with that generator's binary alpha and the 'ALPM' opt-in off) at the same sizes, and ONE rocprofv3
# kernel trace of the batch form at 64 x 2048^2, apart from the timed runs.  Run from the repository root after the build; every GPU step has its
# own time limit and nothing starts after a failure.  The level-0 loop at 64 x 2048^2 runs ZStd level 18 and the 'ALPM' sweep on one stream at a
# time: about a second per frame, 8 x 64 frames -- it comes last and has the longest limit.
#   profiles/encode_files/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/encode_files/encode_vs_loop.py
B=yaik_amd/host/convert_bench
OUT=${1:-profiles/encode_files}
mkdir -p "$OUT"
: > "$OUT/encode_vs_loop.txt"
timeout -k 10 240 python $S 256 512 3 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt" &&
timeout -k 10 300 python $S 64 2048 3 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt" &&
timeout -k 10 300 python $S 4 4096 3 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt" &&
timeout -k 10 300 python $S 256 512 0 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt" &&
timeout -k 10 420 python $S 4 4096 0 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt" &&
timeout -k 10 300 $B 512 256 16 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt" &&
timeout -k 10 420 $B 2048 64 16 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt" &&
timeout -k 10 300 $B 4096 4 16 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt" || exit 1
T=$(mktemp -d)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o encode_files -- python $S 64 2048 3 1 --profile > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; rm -rf "$T"; exit 1; }
find "$T" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_64x2048.csv" \;
rm -rf "$T"
timeout -k 10 1100 python $S 64 2048 0 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/encode_vs_loop.txt"
