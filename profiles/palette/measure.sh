#!/bin/bash
# PaletteCompressor on the device against the host coder at the two sizes, convert_bench at 4096^2 with the option off and on, then ONE rocprofv3
# kernel trace of the 8192^2 call, apart from the timed runs.  Run from the repository root after the build; every GPU step has its own time
# limit and nothing starts after a failure.
#   profiles/palette/measure.sh [output directory, default: next to this script]
set -o pipefail
S=profiles/palette/palette_prof.py
OUT=${1:-profiles/palette}
mkdir -p "$OUT"
: > "$OUT/palette.txt"
timeout -k 10 400 python $S 1 8192 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/palette.txt" || exit 1
timeout -k 10 400 python $S 64 2048 7 --host-frames 4 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/palette.txt" || exit 1
timeout -k 10 300 yaik_amd/host/convert_bench 4096 3 8 0 2>&1 | tee -a "$OUT/palette.txt" || exit 1
timeout -k 10 300 yaik_amd/host/convert_bench 4096 3 8 1 2>&1 | tee -a "$OUT/palette.txt" || exit 1
T=$(mktemp -d)
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o palette -- python $S 1 8192 1 --profile > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
find "$T" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_8192.csv" \;
rm -rf "$T"
