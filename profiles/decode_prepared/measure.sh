#!/bin/bash
# K windows of one image at 8192 and 16384: the loop of single-window decodes against prepare + renders (prepared_vs_loop.py).
# Run from the repository root; every GPU step has its own time limit and nothing starts after a failure.
#   profiles/decode_prepared/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/decode_prepared/prepared_vs_loop.py
OUT=${1:-profiles/decode_prepared}
mkdir -p "$OUT"
: > "$OUT/prepared_vs_loop.txt"
timeout -k 10 240 python $S 8192 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/prepared_vs_loop.txt" &&
timeout -k 10 300 python $S 16384 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/prepared_vs_loop.txt"
