#!/bin/bash
# The alpha stage as one-wave streaming units with the box fold in a kernel of its own, this build against a build of the parent commit,
# in one visit.  Run from the repository root:
#   YK_PARENT_LIB=/path/to/parent/libyaik_hip.so profiles/alpha_stream/measure.sh <output directory> [step ...]
# steps (default: all, in this order): alone bytes timeline_parent timeline_new headline others.  YK_NEW_LIB selects another build of this
# tree (e.g. -DYK_ALPHA_R=8) in place of yaik_amd/libyaik_hip.so.  Kernel traces, counters (--pmc, never with tracing) and end-to-end
# numbers are separate runs; every GPU step has its own time limit, one process uses the GPU at a time and nothing starts after a failure.
set -o pipefail
D=profiles/alpha_stream
OUT=${1:?output directory}; shift
STEPS=${*:-alone bytes timeline_parent timeline_new headline others}
: "${YK_PARENT_LIB:?library of the parent commit}"
NEW_LIB=${YK_NEW_LIB:-$PWD/yaik_amd/libyaik_hip.so}
mkdir -p "$OUT"
T=$(mktemp -d)
lib_of() { if [ "$1" = parent ]; then echo "$YK_PARENT_LIB"; else echo "$NEW_LIB"; fi; }
line() { python3 -c "import sys,json; d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); r=d.get('roofline',{}); print('$1', 'Gpix/s', round(d['value']/1e3,2), 'ms_per_step', d.get('ms_per_step'), 'fused_ms', r.get('kernel_ms'), 'other', r.get('other_kernels_ms'), 'parity', d.get('parity'))"; }
timeline() {    # the two-frame pipeline's kernels: steady-state frames of the default bench command, a trace run of its own (no counters)
    rm -rf "$T/tl"
    YK_LIB=$(lib_of $1) timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$T/tl" -- python bench.py --steps 30 --warmup 5 --no-cpu --no-parity > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
    python3 $D/summarize.py timeline "$T/tl" > "$OUT/timeline_$1.txt" || exit 1
    cat "$OUT/timeline_$1.txt"
}

for step in $STEPS; do
case $step in
alone)      # 1. the stage alone on the four planes of profiles/alpha_early_out/alpha_planes.py
    : > "$OUT/kernel_alone.txt"
    for v in parent new; do
        echo "== $v" >> "$OUT/kernel_alone.txt"
        rm -rf "$T/kt"
        YK_LIB=$(lib_of $v) timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$T/kt" -- python profiles/alpha_early_out/alpha_planes.py 20 a b c d > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
        grep "^plane" "$T/log.txt" >> "$OUT/kernel_alone.txt"
        python3 $D/summarize.py trace "$T/kt" 20 a b c d >> "$OUT/kernel_alone.txt" || exit 1
    done
    cat "$OUT/kernel_alone.txt" ;;
bytes)      # 2. HBM bytes fetched on planes (a) and (b), a --pmc pass of its own
    : > "$OUT/fetch_size.txt"
    for v in parent new; do
        echo "== $v" >> "$OUT/fetch_size.txt"
        rm -rf "$T/pmc"
        YK_LIB=$(lib_of $v) timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$T/pmc" -- python profiles/alpha_early_out/alpha_planes.py 2 a b > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
        python3 $D/summarize.py counter "$T/pmc" 2 a b >> "$OUT/fetch_size.txt" || exit 1
    done
    cat "$OUT/fetch_size.txt" ;;
timeline_parent) timeline parent ;;
timeline_new)    timeline new ;;
headline)   # 3. parent and new alternately, five runs each, parity line included
    : > "$OUT/headline_ab.txt"
    for rep in 1 2 3 4 5; do
        for v in parent new; do
            YK_LIB=$(lib_of $v) timeout -k 10 300 python bench.py --steps 100 --warmup 5 --no-cpu 2> "$T/err.txt" | line "$v run $rep" | tee -a "$OUT/headline_ab.txt" || { tail -20 "$T/err.txt"; exit 1; }
        done
    done ;;
others)     # 4. the other configurations, one alternating pair each
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
