#!/bin/bash
# Host time per call, on a build of the parent commit (YK_PARENT_TREE = its checkout, built) and on this build: bench.py (unmodified; the CPU leg
# and the parity leg are switched off, they time nothing of the library) at its own size and at 512 x 512, where the encode calls are host-bound,
# and the decode of 256 frames of 512 x 512, whose loop form is host-bound (profiles/decode_batch/batch_vs_loop.py, unmodified).  Each in the order parent, new, parent, new, all in one visit, so that the two parent
# runs of a measurement show the spread of one code on this machine.  Run from the repository root after the build; every GPU step has its own
# time limit and nothing starts after a failure.
#   YK_PARENT_TREE=/path/to/parent [ROUNDS=2] profiles/frame_views/measure.sh [output directory, default: next to this script]
set -o pipefail
OUT=${1:-profiles/frame_views}
ROUNDS=${ROUNDS:-2}                                         # parent / new pairs per measurement
[ -n "$YK_PARENT_TREE" ] || { echo "YK_PARENT_TREE is not set"; exit 1; }
mkdir -p "$OUT"
: > "$OUT/ab.txt"
B="bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu --no-parity"
S="profiles/decode_batch/batch_vs_loop.py 256 512 7"
B5="bench.py --gpus 1 --steps 400 --warmup 40 --size 512 --no-cpu --no-parity"
run() {                                                     # run <label> <command ...>
    echo "# $1" | tee -a "$OUT/ab.txt"; shift
    timeout -k 10 240 "$@" 2>&1 | grep -v amdgpu.ids | tee -a "$OUT/ab.txt" || exit 1
}
for round in $(seq 1 $ROUNDS); do
    YK_LIB=$YK_PARENT_TREE/yaik_amd/libyaik_hip.so run "parent build, run $round: $B" python $B
    run "this build, run $round: $B" python $B
done
for round in $(seq 1 $ROUNDS); do
    YK_TREE=$YK_PARENT_TREE run "parent build, run $round: $S" python $S
    run "this build, run $round: $S" python $S
done
for round in $(seq 1 $ROUNDS); do
    YK_LIB=$YK_PARENT_TREE/yaik_amd/libyaik_hip.so run "parent build, run $round: $B5" python $B5
    run "this build, run $round: $B5" python $B5
done
