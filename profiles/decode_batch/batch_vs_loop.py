"""Per-frame decode time of N equally shaped frames from device-resident streams: ONE batch decode against a loop of single-image decodes.
Run from the repository root as
    python profiles/decode_batch/batch_vs_loop.py <frames> <size> [reps] [--loop-only]        e.g. 256 512 | 64 2048 | 2 8192

  loop   per frame: begin + decode_streams (yk_decode_gradient_all_device + yk_decode_1d_device) + image_device into out[f]
  batch  begin_batch + decode_batch_streams + image_batch_device into out, once for all frames

Both read the same streams (every frame encoded on its own, its streams uploaded once into torch tensors) and write the same [N, H, W, 3]
tensor; the script checks that they write the same bytes.  A repetition is `inner` passes over the N frames (at least 256 frames) under a
host clock that ends in a device synchronisation; loop and batch repetitions alternate after a warm-up of each.  Prints per-frame median,
minimum and maximum over the repetitions.

--loop-only times the loop alone: it uses nothing this change added, so with YK_TREE=<a checkout of the parent commit, built> the same script
times the parent's single-image path on the same machine in the same visit."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("YK_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import PASSES, HipTileEncoder
from yaik_amd.synth import synth_planes_torch

args = [a for a in sys.argv[1:] if not a.startswith("--")]
loop_only = "--loop-only" in sys.argv
N, size = int(args[0]), int(args[1])
reps = int(args[2]) if len(args) > 2 else 7
w = h = size
inner = max(1, -(-256 // N))

enc = HipTileEncoder(0)
keep, single, batch = [], [], []
for f in range(N):
    planes = synth_planes_torch(w, h, n_planes=3, seed=9000 + f, device="cuda")
    enc.set_image_u8(planes.permute(1, 2, 0).to(torch.uint8).contiguous())
    enc.encode(3, False, False)
    counts = enc.gradient_counts()
    g = []
    for i, (sx, sy) in enumerate(PASSES):
        bm, rgb = enc.gradient_bitmap(i), enc.gradient_corners(i)
        tb, tr = torch.from_numpy(bm).cuda(), torch.from_numpy(np.concatenate([rgb, np.zeros(16, np.uint8)])).cuda()
        keep += [tb, tr]
        g.append(("g", sx, sy, tb.data_ptr(), bm.size, tr.data_ptr(), rgb.size))
    pix, typ = enc.dynamic_tile_compressor()
    tt, tp = torch.from_numpy(np.concatenate([typ, np.zeros(16, np.uint8)])).cuda(), torch.from_numpy(np.concatenate([pix, np.zeros(16, np.uint8)])).cuda()
    keep += [tt, tp]
    d1 = ("1", tt.data_ptr(), typ.size, tp.data_ptr(), pix.size)
    single.append([c for i, c in enumerate(g) if counts[i]] + [d1])             # what encoder_streams lists: the passes with tiles
    batch.append(g + [d1])                                                       # every pass for every frame
torch.cuda.synchronize()
enc.close()

dec, bdec = HipTileDecoder(0), HipTileDecoder(0)                                # a handle per form: each keeps its buffers from one repetition to the next
out_loop = torch.zeros((N, h, w, 3), dtype=torch.uint8, device="cuda")
out_batch = torch.zeros((N, h, w, 3), dtype=torch.uint8, device="cuda")


def run_loop():
    for f in range(N):
        dec.begin(w, h)
        dec.decode_streams(single[f], sync=False)
        dec.image_device(out_loop[f])


def run_batch():
    bdec.begin_batch(w, h, N)
    bdec.decode_batch_streams(batch, sync=False)
    bdec.image_batch_device(out_batch)


def timed(fn) -> float:
    torch.cuda.synchronize(); dec.synchronize(); bdec.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize(); dec.synchronize(); bdec.synchronize()
    return (time.perf_counter() - t) / (inner * N) * 1e3


forms = [("loop", run_loop)] + ([] if loop_only else [("batch", run_batch)])
for _, fn in forms:                                                              # warm-up: code objects, buffers of both shapes of handle
    for _ in range(2):
        timed(fn)
ms = {name: [] for name, _ in forms}
for _ in range(reps):
    for name, fn in forms:
        ms[name].append(timed(fn))
if not loop_only:
    assert torch.equal(out_loop, out_batch), "batch and loop wrote different pixels"
tree = "YK_TREE build" if os.environ.get("YK_TREE") else "this build"
for name, _ in forms:
    v = ms[name]
    print(f"{N} x {w}x{h} RGB, {tree}, {name:5s}: median {statistics.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; "
          f"{reps} repetitions of {inner * N} frames)", flush=True)
if not loop_only:
    print(f"{N} x {w}x{h} RGB: batch / loop = {statistics.median(ms['batch']) / statistics.median(ms['loop']):.3f}", flush=True)
dec.close(); bdec.close()
