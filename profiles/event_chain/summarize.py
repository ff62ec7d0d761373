"""The frame pipeline's kernels from a rocprofv3 --kernel-trace output directory of the default bench command (the timeline form of
profiles/alpha_early_out/summarize.py, plus the gaps as numbers):
    python profiles/event_chain/summarize.py timeline <dir>   -> the kernels of five steady-state frames, times relative to the start of a fused kernel,
                                                                 then the gap between the end of a fused kernel and the start of the next one and the
                                                                 dead stream time in front of every kernel kind, over the middle half of the trace"""
import collections, csv, glob, statistics, sys

mode, d = sys.argv[1], sys.argv[2]
assert mode == "timeline", mode
rows = []
for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
    rows += [r for r in csv.DictReader(open(f)) if "yk_" in r["Kernel_Name"] and not any(s in r["Kernel_Name"] for s in ("roof", "qtab", "deftab"))]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: r["Kernel_Name"].split("(")[0].split("<")[0]
fused = [i for i, r in enumerate(rows) if "encode2" in r["Kernel_Name"]]
assert len(fused) > 12, len(fused)
a, b = fused[len(fused) // 2], fused[len(fused) // 2 + 5]
t0 = int(rows[a]["Start_Timestamp"])
for r in rows[a - 6:b + 1]:
    s, e = int(r["Start_Timestamp"]) - t0, int(r["End_Timestamp"]) - t0
    print(f'{name(r)[:28]:28s} q{r.get("Queue_Id", "?"):>3s} start {s / 1e3:9.1f} us  end {e / 1e3:9.1f} us  dur {(e - s) / 1e3:7.1f}')

lo, hi = len(fused) // 4, len(fused) * 3 // 4
gaps = [(int(rows[fused[k + 1]]["Start_Timestamp"]) - int(rows[fused[k]]["End_Timestamp"])) / 1e3 for k in range(lo, hi)]
durs = [(int(rows[fused[k]]["End_Timestamp"]) - int(rows[fused[k]]["Start_Timestamp"])) / 1e3 for k in range(lo, hi)]
print(f"\nfused end -> next fused start, {len(gaps)} frames: mean {statistics.mean(gaps):.1f} us  median {statistics.median(gaps):.1f}  min {min(gaps):.1f}  max {max(gaps):.1f}"
      f"   (fused kernel: mean {statistics.mean(durs):.1f} us; frame = {statistics.mean(durs) + statistics.mean(gaps):.1f} us)")
# dead time in front of a kernel on its own queue: its start minus the end of the kernel before it on that queue
last, dead = {}, collections.defaultdict(list)
for i, r in enumerate(rows):
    q = r.get("Queue_Id", "?")
    if q in last and fused[lo] <= i <= fused[hi]:
        p = last[q]
        dead[f"{name(p)} -> {name(r)}"].append((int(r["Start_Timestamp"]) - int(p["End_Timestamp"])) / 1e3)
    last[q] = r
for k, v in sorted(dead.items()):
    print(f"same queue, {k:58s} n {len(v):3d}  median {statistics.median(v):7.1f} us  min {min(v):7.1f}")
