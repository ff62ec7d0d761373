"""yk_alpha_kernel per plane from a rocprofv3 output directory of alpha_planes.py:
    python profiles/alpha_early_out/summarize.py trace   <dir> <reps> <plane> ...   -> duration (us): min / median of the REPS timed launches
    python profiles/alpha_early_out/summarize.py counter <dir> <reps> <plane> ...   -> FETCH_SIZE of the last launch: raw KB and bytes (x1024, x2 on gfx950)
    python profiles/alpha_early_out/summarize.py timeline <dir>                     -> the kernels of five steady-state frames of a bench trace,
                                                                                       times relative to the start of a fused kernel (the form of tools/ktimeline.sh)
alpha_planes.py issues reps + 3 launches per plane: two to warm up, the REPS timed ones, one of its closing mip_prefilter."""
import collections, csv, glob, statistics, sys

mode, d = sys.argv[1], sys.argv[2]
if mode == "timeline":
    rows = []
    for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "yk_" in r["Kernel_Name"] and not any(s in r["Kernel_Name"] for s in ("roof", "qtab", "deftab"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    fused = [i for i, r in enumerate(rows) if "encode2" in r["Kernel_Name"]]
    assert len(fused) > 12, len(fused)
    a, b = fused[len(fused) // 2], fused[len(fused) // 2 + 5]
    t0 = int(rows[a]["Start_Timestamp"])
    for r in rows[a - 6:b + 1]:
        s, e = int(r["Start_Timestamp"]) - t0, int(r["End_Timestamp"]) - t0
        print(f'{r["Kernel_Name"].split("(")[0][:28]:28s} q{r.get("Queue_Id", "?"):>3s} start {s / 1e3:9.1f} us  end {e / 1e3:9.1f} us  dur {(e - s) / 1e3:7.1f}')
    sys.exit(0)
reps, planes = int(sys.argv[3]), sys.argv[4:]
per = reps + 3
if mode == "trace":
    rows = []
    for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "yk_alpha_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == per * len(planes), (len(rows), per, planes)
    for i, p in enumerate(planes):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * per + 2:i * per + 2 + reps]]
        print(f"plane {p}: yk_alpha_kernel min {min(us):6.1f} us  median {statistics.median(us):6.1f} us  max {max(us):6.1f} us  ({reps} launches)")
else:
    acc = collections.defaultdict(float)
    for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "yk_alpha_kernel" in r["Kernel_Name"] and r["Counter_Name"] == "FETCH_SIZE":
                acc[int(r["Dispatch_Id"])] += float(r["Counter_Value"])
    ids = sorted(acc)
    assert len(ids) == per * len(planes), (len(ids), per, planes)
    for i, p in enumerate(planes):
        kb = acc[ids[i * per + per - 2]]
        print(f"plane {p}: FETCH_SIZE {kb:.0f} KB -> {kb * 1024 * 2 / 1e6:.1f} MB (x1024, x2 on gfx950)")
