#!/bin/bash
# The fused encode kernel's whole-block instantiation, this build against a build of the parent commit, in one visit.  Run
# from the repository root:
#   YK_PARENT_LIB=/path/to/parent/libyaik_hip.so profiles/whole_blocks/measure.sh <output directory> [step ...]
# steps (default: all, in this order): classes headline others.  YK_NEW_LIB selects another build of this tree in place of
# yaik_amd/libyaik_hip.so; YK_STEP_LIBS="name=/path/lib.so ..." adds builds of single items to the `classes` step (the stop rules).  Counters
# (--pmc, never with tracing) and end-to-end numbers are separate runs; every GPU step has its own time limit, one process uses the GPU at a
# time and nothing starts after a failure.
set -o pipefail
OUT=${1:?output directory}; shift
STEPS=${*:-classes headline others}
: "${YK_PARENT_LIB:?library of the parent commit}"
NEW_LIB=${YK_NEW_LIB:-$PWD/yaik_amd/libyaik_hip.so}
mkdir -p "$OUT"
T=$(mktemp -d)
lib_of() {
    case $1 in
    parent|parent2) echo "$YK_PARENT_LIB" ;;
    new) echo "$NEW_LIB" ;;
    *) for kv in $YK_STEP_LIBS; do [ "${kv%%=*}" = "$1" ] && echo "${kv#*=}"; done ;;
    esac
}
line() { python3 -c "import sys,json; d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); r=d.get('roofline',{}); print('$1', 'Gpix/s', round(d['value']/1e3,2), 'ms_per_step', d.get('ms_per_step'), 'fused_ms', r.get('kernel_ms'), 'fused_alone_ms', (r.get('kernel_alone') or {}).get('kernel_ms'), 'parity', d.get('parity'))"; }

for step in $STEPS; do
case $step in
classes)    # 1. wave-instructions of the fused kernel per strip and content class (tools/gpu_class_pmc.py: whole 8192^2 frames of one class, which qualify for the whole-block kernel; empty = all noise, all alpha-rejected: the fixed cost), a --pmc pass per run
    : > "$OUT/valu_per_strip_by_class.txt"
    for v in parent parent2 $(for kv in $YK_STEP_LIBS; do echo "${kv%%=*}"; done) new; do      # the parent twice first: what two runs of one library differ by
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
            tail -1 "$OUT/valu_per_strip_by_class.txt"
        done
    done ;;
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
def rule(key, better):
    p = [val(w, key) for w in rows if w[0] == "parent"]; n = [val(w, key) for w in rows if w[0] == "new"]
    mp, mn = sum(p) / len(p), sum(n) / len(n)
    s = max(p) - min(p)
    apart = min(n) > max(p) if better > 0 else max(n) < min(p)
    d = (mn - mp) * better
    print(f"# {key}: parent {p} mean {mp:.4f} spread {s:.4f} | new {n} mean {mn:.4f} spread {max(n) - min(n):.4f} | new / parent {mn / mp:.4f}")
    print(f"#   rule (DESIGN 8.2): every new run better than every parent run: {apart}; difference of the means {d:.4f} = {d / s if s else float('inf'):.1f} x the parent's spread -> {'met' if apart and d >= 2 * s else 'NOT met'}")
rule("Gpix/s", +1); rule("fused_ms", -1); rule("fused_alone_ms", -1)
print(f"# all ten bit-exact: {all('bit-exact' in ' '.join(w) for w in rows)}")
PY
    ;;
others)     # 3. the other configurations, one alternating pair each (--size 2048 --batch 32 stays on the general kernel: it must not move)
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
