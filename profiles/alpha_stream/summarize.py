"""The alpha stage (yk_alpha_kernel + yk_alpha_box_kernel; the parent commit has the first alone) from rocprofv3 output directories:
    python profiles/alpha_stream/summarize.py trace   <dir> <reps> <plane> ...   -> per plane of profiles/alpha_early_out/alpha_planes.py: start of the alpha
                                                                                     kernel to the end of the fold behind it (us), min / median / max of the
                                                                                     REPS timed launches, and the fold kernel's own median
    python profiles/alpha_stream/summarize.py counter <dir> <reps> <plane> ...   -> FETCH_SIZE of the last launch, both kernels: bytes (x1024, x2 on gfx950)
    python profiles/alpha_stream/summarize.py timeline <dir>                     -> profiles/event_chain/summarize.py's view of a bench trace (kernels of five
                                                                                     frames, gap between fused kernels, dead stream time) and where the alpha
                                                                                     stage ends relative to the end of the fused kernel it ran beside
alpha_planes.py issues reps + 3 launches per plane: two to warm up, the REPS timed ones, one of its closing mip_prefilter."""
import collections, csv, glob, os, runpy, statistics, sys

mode, d = sys.argv[1], sys.argv[2]
S, E = (lambda r: int(r["Start_Timestamp"])), (lambda r: int(r["End_Timestamp"]))


def kernel_rows(pattern):
    rows = []
    for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if pattern(r["Kernel_Name"])]
    rows.sort(key=S)
    return rows


if mode == "timeline":
    sys.argv = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "event_chain", "summarize.py"), "timeline", d]
    runpy.run_path(sys.argv[0], run_name="__main__")
    rows = kernel_rows(lambda n: "yk_alpha" in n or "encode2" in n)
    fused = [r for r in rows if "encode2" in r["Kernel_Name"]]
    # a stage = the alpha kernel and the fold behind it on the same queue (the parent commit: the alpha kernel alone)
    has_fold = any("yk_alpha_box_kernel" in r["Kernel_Name"] for r in rows)
    stages, open_ = [], {}
    for r in rows:
        q = r.get("Queue_Id", "?")
        if "yk_alpha_kernel" in r["Kernel_Name"]:
            if has_fold:
                open_.setdefault(q, S(r))
            else:
                stages.append((S(r), E(r)))
        elif "yk_alpha_box_kernel" in r["Kernel_Name"] and q in open_:
            stages.append((open_.pop(q), E(r)))
    lo, hi = S(fused[len(fused) // 4]), S(fused[len(fused) * 3 // 4])
    rel, into, dur = [], [], []
    for s0, e0 in stages:
        if not lo <= s0 <= hi:
            continue
        beside = [r for r in fused if S(r) <= s0 < E(r)]                      # the other frame's fused kernel, running when this stage starts
        if not beside:
            continue
        rel.append((e0 - E(beside[0])) / 1e3); into.append((e0 - S(beside[0])) / 1e3); dur.append((e0 - s0) / 1e3)
    print(f"alpha stage ({'alpha + fold' if has_fold else 'alpha kernel'}), {len(rel)} frames: ends {statistics.mean(rel):+.1f} us relative to the end of the other frame's fused kernel "
          f"(min {min(rel):+.1f}, max {max(rel):+.1f}), {statistics.mean(into):.1f} us after its start; start to end {statistics.mean(dur):.1f} us")
    sys.exit(0)
reps, planes = int(sys.argv[3]), sys.argv[4:]
per = reps + 3
if mode == "trace":
    alpha, fold = kernel_rows(lambda n: "yk_alpha_kernel" in n), kernel_rows(lambda n: "yk_alpha_box_kernel" in n)
    assert len(alpha) == per * len(planes) and len(fold) in (0, len(alpha)), (len(alpha), len(fold), per, planes)
    for i, p in enumerate(planes):
        sel = range(i * per + 2, i * per + 2 + reps)
        us = [((E(fold[k]) if fold else E(alpha[k])) - S(alpha[k])) / 1e3 for k in sel]
        extra = f"  fold kernel median {statistics.median((E(fold[k]) - S(fold[k])) / 1e3 for k in sel):4.1f} us" if fold else ""
        print(f"plane {p}: alpha stage min {min(us):6.1f} us  median {statistics.median(us):6.1f} us  max {max(us):6.1f} us  ({reps} launches){extra}")
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
        print(f"plane {p}: yk_alpha_kernel FETCH_SIZE {kb:.0f} KB -> {kb * 1024 * 2 / 1e6:.1f} MB (x1024, x2 on gfx950)")
