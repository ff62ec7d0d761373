#!/bin/bash
# PaletteDecompressor on the device against the host coder at the two sizes; decode_batch_from_encoder end to end with palette off and on at the
# three sizes, and the default path on a build of the parent commit (YK_PARENT_TREE = its checkout, built) in the same visit; then ONE rocprofv3
# kernel trace of the 8192^2 call, apart from the timed runs.  Run from the repository root after the build; every GPU step has its own time
# limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/palette_decode/measure.sh [output directory, default: next to this script]
set -o pipefail
D=profiles/palette_decode
OUT=${1:-$D}
mkdir -p "$OUT"
: > "$OUT/palette_decode.txt"
timeout -k 10 300 python $D/palette_dec_prof.py 1 8192 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/palette_decode.txt" || exit 1
timeout -k 10 300 python $D/palette_dec_prof.py 64 2048 7 --host-frames 4 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/palette_decode.txt" || exit 1
for c in "256 512" "64 2048" "2 8192"; do
    if [ -n "$YK_PARENT_TREE" ]; then
        YK_TREE=$YK_PARENT_TREE timeout -k 10 240 python $D/e2e.py $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/palette_decode.txt" || exit 1
    fi
    timeout -k 10 240 python $D/e2e.py $c 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/palette_decode.txt" || exit 1
    timeout -k 10 240 python $D/e2e.py $c 7 --palette 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/palette_decode.txt" || exit 1
done
T=$(mktemp -d)
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o palette_decode -- python $D/palette_dec_prof.py 1 8192 1 --profile > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
find "$T" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_8192.csv" \;
rm -rf "$T"
