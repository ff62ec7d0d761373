"""Per-frame cost of building the corner and 1-D streams of an encoded batch: HipTileDecoder.encoder_batch_streams(enc) (yk_encode_streams_batch:
one launch per kernel, one read-back, no copies) against encoder_batch_streams(enc, per_frame=True) (the loop over select_frame: nine stream
operations, two read-backs and nine device-to-device copies per frame).  Run from the repository root as
    python profiles/encode_streams_batch/batch_vs_per_frame.py <frames> <size> [reps]          e.g. 256 512 | 64 2048 | 2 8192

The encoder is encoded once, before the clock starts.  A repetition is one call under a host clock that ends in a device synchronisation; batch and
per-frame repetitions alternate after a warm-up of each.  Prints per-frame median, minimum and maximum over the repetitions, the stage timers
(yk_stage_ms) of one batch call, and asserts that the two forms' streams are byte-equal."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

N, size = int(sys.argv[1]), int(sys.argv[2])
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
w = h = size

enc = HipTileEncoder(0)
frames = torch.empty((N, h, w, 3), dtype=torch.uint8, device="cuda")
for f in range(N):
    frames[f] = synth_planes_torch(w, h, n_planes=3, seed=9000 + f, device="cuda").permute(1, 2, 0).to(torch.uint8)
torch.cuda.synchronize()
enc.set_batch_u8(frames)
enc.encode_batch(3, False)
enc.synchronize()

db, dl = HipTileDecoder(0), HipTileDecoder(0)                                    # a handle per form: each keeps what it allocates between repetitions
db.begin_batch(w, h, N); dl.begin_batch(w, h, N)
db.synchronize(); dl.synchronize()
last = {}


def run_batch():
    last["batch"] = db.encoder_batch_streams(enc)


def run_loop():
    last["loop"] = dl.encoder_batch_streams(enc, per_frame=True)


def timed(fn) -> float:
    torch.cuda.synchronize(); enc.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(); enc.synchronize()
    return (time.perf_counter() - t) / N * 1e3


forms = [("per-frame", run_loop), ("batch", run_batch)]
for _, fn in forms:
    for _ in range(2):
        timed(fn)
ms = {name: [] for name, _ in forms}
for _ in range(reps):
    for name, fn in forms:
        ms[name].append(timed(fn))


def fetch(ptr, n):
    out = np.empty(n, dtype=np.uint8)
    if n:
        rc = enc._L.yk_device_download(enc._h, out.ctypes.data, C.c_void_p(ptr), n)
        assert rc == 0, rc
    return out


total = 0
for f in range(N):                                                               # both forms' last results are still in HBM: the same bytes, stream by stream
    for a, b in zip(last["batch"][f], last["loop"][f]):
        assert a[:3] == b[:3] and (a[4], a[6]) == (b[4], b[6]) if a[0] == "g" else (a[2], a[4]) == (b[2], b[4]), (f, a, b)
        pairs = [(a[5], b[5], a[6])] if a[0] == "g" else [(a[1], b[1], a[2]), (a[3], b[3], a[4])]
        for pa, pb, n in pairs:
            assert np.array_equal(fetch(pa, n), fetch(pb, n)), (f, a[:3])
            total += n
print(f"{N} x {w}x{h} RGB: the two forms' streams are byte-equal ({total} bytes over {N} frames)", flush=True)
for name, _ in forms:
    v = ms[name]
    print(f"{N} x {w}x{h} RGB, {name:9s}: median {statistics.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; {reps} repetitions)", flush=True)
print(f"{N} x {w}x{h} RGB: batch / per-frame = {statistics.median(ms['batch']) / statistics.median(ms['per-frame']):.3f}", flush=True)
for st in (0, 1, 2):
    enc.stage_ms(st)
enc.streams_batch()
enc.synchronize()
names = {0: "CORNERS (spans the read-back)", 2: "RANGE1D_PACK", 1: "RANGE1D"}
print(f"{N} x {w}x{h} RGB, stage timers of one batch call: " + ", ".join(f"{names[st]} {enc.stage_ms(st)[0]:.3f} ms" for st in (0, 2, 1)), flush=True)
db.close(); dl.close(); enc.close()
