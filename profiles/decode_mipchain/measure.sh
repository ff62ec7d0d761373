#!/bin/bash
# A whole mip chain from one call against the four output calls plus a reduction in torch (chain_vs_calls.py) at 8192, 16384 and for a batch of
# 256 x 512 x 512; then bench.py --stage decode on a build of the parent commit (YK_PARENT_TREE = its checkout, built) and on this build,
# alternating, five each.  Run from the repository root; every GPU step has its own time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent profiles/decode_mipchain/measure.sh [output directory, default: next to this script]
#   YK_SKIP_CHAIN=1 runs the bench comparison alone
set -o pipefail
S=profiles/decode_mipchain/chain_vs_calls.py
OUT=${1:-profiles/decode_mipchain}
mkdir -p "$OUT"
if [ -z "$YK_SKIP_CHAIN" ]; then
    : > "$OUT/chain_vs_calls.txt"
    timeout -k 10 240 python $S image 8192 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/chain_vs_calls.txt" &&
    timeout -k 10 300 python $S image 16384 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/chain_vs_calls.txt" &&
    timeout -k 10 240 python $S batch 256 512 7 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/chain_vs_calls.txt" || exit 1
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
