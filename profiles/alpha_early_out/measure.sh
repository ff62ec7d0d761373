#!/bin/bash
# The alpha kernel's early-out, this build against a build of the parent commit, in one visit.  Run from the repository root:
#   YK_PARENT_LIB=/path/to/parent/libyaik_hip.so profiles/alpha_early_out/measure.sh <output directory> [step ...]
# steps (default: all, in this order): alone bytes timeline headline others.  Kernel traces, counters (--pmc, never with tracing) and
# end-to-end numbers are separate runs; every GPU step has its own time limit and nothing starts after a failure.
set -o pipefail
D=profiles/alpha_early_out
OUT=${1:?output directory}; shift
STEPS=${*:-alone bytes timeline headline others}
: "${YK_PARENT_LIB:?library of the parent commit}"
NEW_LIB=$PWD/yaik_amd/libyaik_hip.so
mkdir -p "$OUT"
T=$(mktemp -d)
lib_of() { if [ "$1" = parent ]; then echo "$YK_PARENT_LIB"; else echo "$NEW_LIB"; fi; }
line() { python3 -c "import sys,json; d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); r=d.get('roofline',{}); print('$1', 'Gpix/s', round(d['value']/1e3,2), 'ms_per_step', d['ms_per_step'], 'fused_ms', r.get('kernel_ms'), 'other', r.get('other_kernels_ms'), 'parity', d.get('parity'))"; }

for step in $STEPS; do
case $step in
alone)      # 1. the kernel alone on the four planes
    : > "$OUT/kernel_alone.txt"
    for v in parent new; do
        echo "== $v" >> "$OUT/kernel_alone.txt"
        rm -rf "$T/kt"
        YK_LIB=$(lib_of $v) timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$T/kt" -- python $D/alpha_planes.py 20 a b c d > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
        grep "^plane" "$T/log.txt" >> "$OUT/kernel_alone.txt"
        python3 $D/summarize.py trace "$T/kt" 20 a b c d >> "$OUT/kernel_alone.txt" || exit 1
    done
    cat "$OUT/kernel_alone.txt" ;;
bytes)      # 2. HBM bytes fetched, a --pmc pass of its own
    : > "$OUT/fetch_size.txt"
    for v in parent new; do
        echo "== $v" >> "$OUT/fetch_size.txt"
        rm -rf "$T/pmc"
        YK_LIB=$(lib_of $v) timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$T/pmc" -- python $D/alpha_planes.py 2 a b c d > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
        python3 $D/summarize.py counter "$T/pmc" 2 a b c d >> "$OUT/fetch_size.txt" || exit 1
    done
    cat "$OUT/fetch_size.txt" ;;
timeline)   # 3. the two-frame pipeline's kernels: a few steady-state frames of the default bench command
    for v in parent new; do
        rm -rf "$T/tl"
        YK_LIB=$(lib_of $v) timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$T/tl" -- python bench.py --steps 30 --warmup 5 --no-cpu --no-parity > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
        python3 $D/summarize.py timeline "$T/tl" > "$OUT/timeline_$v.txt" || exit 1
    done
    cat "$OUT/timeline_parent.txt" "$OUT/timeline_new.txt" ;;
headline)   # 4. parent and new alternately, five runs each
    : > "$OUT/headline_ab.txt"
    for rep in 1 2 3 4 5; do
        for v in parent new; do
            YK_LIB=$(lib_of $v) timeout -k 10 300 python bench.py --steps 100 --warmup 5 --no-cpu 2> "$T/err.txt" | line "$v run $rep" | tee -a "$OUT/headline_ab.txt" || { tail -20 "$T/err.txt"; exit 1; }
        done
    done ;;
others)     # 5. the other configurations, one run each
    : > "$OUT/other_configs.txt"
    for cfg in "--size 2048 --batch 32" "--graph" "--in-flight 1" "--stage all"; do
        for v in parent new; do
            YK_LIB=$(lib_of $v) timeout -k 10 300 python bench.py --steps 100 --warmup 5 --no-cpu --no-parity $cfg 2> "$T/err.txt" | line "$v [$cfg]" | tee -a "$OUT/other_configs.txt" || { tail -20 "$T/err.txt"; exit 1; }
        done
    done ;;
*) echo "unknown step $step"; exit 2 ;;
esac
done
rm -rf "$T"
