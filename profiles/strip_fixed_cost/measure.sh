#!/bin/bash
# What a strip of the fused encode kernel pays outside its pixel loops, this build against a build of the parent commit, in one visit.  Run from
# the repository root:
#   YK_PARENT_LIB=/path/to/parent/libyaik_hip.so profiles/strip_fixed_cost/measure.sh <output directory> [step ...]
# steps (default: all, in this order): classes headline others.  YK_NEW_LIB selects another build of this tree in place of
# yaik_amd/libyaik_hip.so.  Counters (--pmc, never with tracing) and end-to-end numbers are separate runs; every GPU step has its own time
# limit, one process uses the GPU at a time and nothing starts after a failure.
set -o pipefail
OUT=${1:?output directory}; shift
STEPS=${*:-classes headline others}
: "${YK_PARENT_LIB:?library of the parent commit}"
NEW_LIB=${YK_NEW_LIB:-$PWD/yaik_amd/libyaik_hip.so}
mkdir -p "$OUT"
T=$(mktemp -d)
lib_of() { if [ "$1" = parent ] || [ "$1" = parent2 ]; then echo "$YK_PARENT_LIB"; else echo "$NEW_LIB"; fi; }
line() { python3 -c "import sys,json; d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); r=d.get('roofline',{}); print('$1', 'Gpix/s', round(d['value']/1e3,2), 'ms_per_step', d.get('ms_per_step'), 'fused_ms', r.get('kernel_ms'), 'fused_alone_ms', (r.get('kernel_alone') or {}).get('kernel_ms'), 'parity', d.get('parity'))"; }

for step in $STEPS; do
case $step in
classes)    # 1. wave-instructions of the fused kernel per strip and content class (tools/gpu_class_pmc.py: whole 8192^2 frames of one class; empty = all noise, all alpha-rejected: the fixed cost), a --pmc pass per run
    : > "$OUT/valu_per_strip_by_class.txt"
    for v in parent parent2 new; do                                 # the parent twice first: what two runs of one library differ by
        for cls in empty ramp noise mild border frame; do
            rm -rf "$T/pmc"
            YK_LIB=$(lib_of $v) timeout -k 10 150 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM --output-format csv -d "$T/pmc" -- python3 tools/gpu_class_pmc.py $cls 0 > "$T/log.txt" 2>&1 || { tail -20 "$T/log.txt"; exit 1; }
            python3 - "$T/pmc" $v $cls <<'PY' >> "$OUT/valu_per_strip_by_class.txt" || exit 1
import csv, glob, collections, sys
d_, v, cls = sys.argv[1:4]
acc = collections.defaultdict(lambda: collections.defaultdict(float))
for f in glob.glob(d_ + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "yk_encode2" in r["Kernel_Name"]:
            acc[r["Dispatch_Id"]][r["Counter_Name"]] += float(r["Counter_Value"])
d = list(acc.values())[-1]
w = d["SQ_WAVES"]
print(v, cls, "waves", int(w), {k: round(x / w, 1) for k, x in sorted(d.items()) if k != "SQ_WAVES"})
PY
            grep "fused kernel" "$T/log.txt" | sed "s/^/$v (under the counters) /" >> "$OUT/valu_per_strip_by_class.txt"
        done
    done
    cat "$OUT/valu_per_strip_by_class.txt" ;;
headline)   # 2. parent and new alternately, five runs each, parity line included; the rule of DESIGN 8.2 is evaluated underneath
    : > "$OUT/headline_ab.txt"
    for rep in 1 2 3 4 5; do
        for v in parent new; do
            YK_LIB=$(lib_of $v) timeout -k 10 300 python bench.py --steps 100 --warmup 5 --no-cpu 2> "$T/err.txt" | line "$v run $rep" | tee -a "$OUT/headline_ab.txt" || { tail -20 "$T/err.txt"; exit 1; }
        done
    done
    python3 - "$OUT/headline_ab.txt" <<'PY' | tee -a "$OUT/headline_ab.txt"
import sys
rows = [l.split() for l in open(sys.argv[1]) if " run " in l]
val = lambda w, key: float(w[w.index(key) + 1])
for key in ("Gpix/s", "fused_ms", "fused_alone_ms"):
    p = [val(w, key) for w in rows if w[0] == "parent"]; n = [val(w, key) for w in rows if w[0] == "new"]
    mp, mn = sum(p) / len(p), sum(n) / len(n)
    print(f"# {key}: parent {p} mean {mp:.4f} spread {max(p) - min(p):.4f} | new {n} mean {mn:.4f} spread {max(n) - min(n):.4f} | new / parent {mn / mp:.4f}")
p = [val(w, "Gpix/s") for w in rows if w[0] == "parent"]; n = [val(w, "Gpix/s") for w in rows if w[0] == "new"]
d, s = sum(n) / len(n) - sum(p) / len(p), max(p) - min(p)
print(f"# rule (DESIGN 8.2): every new run above every parent run: {min(n) > max(p)}; difference of the means {d:.3f} Gpix/s = {d / s if s else float('inf'):.1f} x the parent's spread ({s:.3f}); all ten bit-exact: {all('bit-exact' in ' '.join(w) for w in rows)}")
PY
    ;;
others)     # 3. the other configurations, one alternating pair each
    : > "$OUT/other_configs.txt"
    for cfg in "--in-flight 1" "--size 2048 --batch 32" "--graph" "--stage all"; do
        for v in parent new; do
            YK_LIB=$(lib_of $v) timeout -k 10 300 python bench.py --steps 100 --warmup 5 --no-cpu --no-parity $cfg 2> "$T/err.txt" | line "$v [$cfg]" | tee -a "$OUT/other_configs.txt" || { tail -20 "$T/err.txt"; exit 1; }
        done
    done ;;
*) echo "unknown step $step"; exit 2 ;;
esac
done
rm -rf "$T"
