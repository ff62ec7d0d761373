#!/bin/bash
# decode_files_device against the loop of decode_file_device at the three sizes, then ONE rocprofv3 kernel trace of the batch form at 64 x 2048^2,
# apart from the timed runs.  Run from the repository root after the build; every GPU step has its own time limit and nothing starts after a failure.
#   profiles/decode_files/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_files/batch_vs_loop.py
OUT=${1:-profiles/decode_files}
mkdir -p "$OUT"
: > "$OUT/batch_vs_loop.txt"
timeout -k 10 240 python $S 256 512 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_loop.txt" &&
timeout -k 10 300 python $S 64 2048 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_loop.txt" &&
timeout -k 10 300 python $S 2 8192 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_loop.txt" || exit 1
T=$(mktemp -d)
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$T" -o decode_files -- python $S 64 2048 1 --profile > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
find "$T" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_64x2048.csv" \;
rm -rf "$T"
