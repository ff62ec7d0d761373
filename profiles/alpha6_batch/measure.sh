#!/bin/bash
# yk_alpha_values_mask_batch against the loop of single-image calls (yk_alpha_reject + yk_alpha_finish + yk_alpha_values(0)) at the three sizes,
# and ONE rocprofv3 kernel trace of the batch form at 256 x 512^2, apart from the timed runs.  Run from the repository root after the build; every
# GPU step has its own time limit and nothing starts after a failure.  The scripts start no worker threads.
#   profiles/alpha6_batch/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/alpha6_batch/batch_vs_loop.py
OUT=${1:-profiles/alpha6_batch}
mkdir -p "$OUT"
: > "$OUT/batch_vs_loop.txt"
timeout -k 10 240 python $S 256 512 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_loop.txt" &&
timeout -k 10 300 python $S 64 2048 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_loop.txt" &&
timeout -k 10 300 python $S 4 4096 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/batch_vs_loop.txt" || exit 1
T=$(mktemp -d)
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o alpha6_batch -- python $S 256 512 1 --profile > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; rm -rf "$T"; exit 1; }
find "$T" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_256x512.csv" \;
rm -rf "$T"
