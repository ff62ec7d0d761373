#!/bin/bash
# The event chain between the frames' fused kernels, this build against a build of the parent commit, in one visit.  Run from the repository root:
#   YK_PARENT_LIB=/path/to/parent/libyaik_hip.so profiles/event_chain/measure.sh <output directory> [step ...]
# steps (default: all, in this order): packets timeline_parent timeline_new headline others.  packets needs profiles/event_chain/packet_cost
# (hipcc -O2 --offload-arch=gfx950 -o profiles/event_chain/packet_cost profiles/event_chain/packet_cost.hip).  Kernel traces and end-to-end
# numbers are separate runs; every GPU step has its own time limit, one process uses the GPU at a time and nothing starts after a failure.
set -o pipefail
D=profiles/event_chain
OUT=${1:?output directory}; shift
STEPS=${*:-packets timeline_parent timeline_new headline others}
: "${YK_PARENT_LIB:?library of the parent commit}"
NEW_LIB=$PWD/yaik_amd/libyaik_hip.so
mkdir -p "$OUT"
T=$(mktemp -d)
lib_of() { if [ "$1" = parent ]; then echo "$YK_PARENT_LIB"; else echo "$NEW_LIB"; fi; }
line() { python3 -c "import sys,json; d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); r=d.get('roofline',{}); print('$1', 'Gpix/s', round(d['value']/1e3,2), 'ms_per_step', d.get('ms_per_step'), 'fused_ms', r.get('kernel_ms'), 'other', r.get('other_kernels_ms'), 'parity', d.get('parity'))"; }
timeline() {    # the two-frame pipeline's kernels: a few steady-state frames of the default bench command, a trace run of its own
    rm -rf "$T/tl"
    YK_LIB=$(lib_of $1) timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$T/tl" -- python bench.py --steps 30 --warmup 5 --no-cpu --no-parity > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
    python3 $D/summarize.py timeline "$T/tl" > "$OUT/timeline_$1.txt" || exit 1
    cat "$OUT/timeline_$1.txt"
}

for step in $STEPS; do
case $step in
packets)    # 1. what one stream operation between two kernels costs, and what dispatch-bound events report
    timeout -k 10 120 $D/packet_cost 200 > "$OUT/packet_cost.txt" 2> "$T/err.txt" || { cat "$OUT/packet_cost.txt"; tail -20 "$T/err.txt"; exit 1; }
    cat "$OUT/packet_cost.txt" ;;
timeline_parent) timeline parent ;;
timeline_new)    timeline new ;;
headline)   # 2. parent and new alternately, five runs each
    : > "$OUT/headline_ab.txt"
    for rep in 1 2 3 4 5; do
        for v in parent new; do
            YK_LIB=$(lib_of $v) timeout -k 10 300 python bench.py --steps 100 --warmup 5 --no-cpu 2> "$T/err.txt" | line "$v run $rep" | tee -a "$OUT/headline_ab.txt" || { tail -20 "$T/err.txt"; exit 1; }
        done
    done ;;
others)     # 3. the other configurations, one pair each
    : > "$OUT/other_configs.txt"
    for cfg in "--in-flight 1" "--size 2048 --batch 32" "--graph" "--stage all"; do
        for v in parent new; do
            YK_LIB=$(lib_of $v) timeout -k 10 300 python bench.py --steps 100 --warmup 5 --no-cpu $cfg 2> "$T/err.txt" | line "$v [$cfg]" | tee -a "$OUT/other_configs.txt" || { tail -20 "$T/err.txt"; exit 1; }
        done
    done ;;
*) echo "unknown step $step"; exit 2 ;;
esac
done
rm -rf "$T"
