"""A window of every frame of a batch against the whole batch decode + crop, from device-resident streams of N encoded frames.  Run from the
repository root as
    python profiles/decode_batch_window/window_vs_whole.py <frames> <size> <window> [reps] [--whole-only]     e.g. 256 512 224 | 64 2048 512 | 2 8192 512

  whole+crop  begin_batch + decode_batch_streams + image_batch_device + a torch gather of every frame's crop into [N, wh, ww, 3]   (what a caller did before)
  windows     begin_batch + set_batch_windows + decode_batch_streams + image_batch_windows_device                                   (yk_decode_set_batch_windows)

with one random 8-aligned origin per frame from a fixed seed.  Both forms read the same streams (every frame encoded on its own, its streams
uploaded once into torch tensors, as profiles/decode_batch/batch_vs_loop.py does) and the script checks that they produce the same bytes.  A
repetition is `inner` batches (at least 256 frames) under a host clock that ends in a device synchronisation; the two forms alternate after a
warm-up of each.  Prints per-frame median, minimum and maximum over the repetitions, and for the window form the stage intervals (gradient, 1-D,
de-tile: yk_stage_ms) per batch, which show the map-sized share that stays.

--whole-only times the whole form alone: it uses nothing this change added, so with YK_TREE=<a checkout of the parent commit, built> the same
script times the parent's path on the same machine in the same visit."""
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
whole_only = "--whole-only" in sys.argv
N, size, win = int(args[0]), int(args[1]), int(args[2])
reps = int(args[3]) if len(args) > 3 else 7
w = h = size
inner = max(1, -(-256 // N))
ST_GRADIENT, ST_1D, ST_DETILE = 3, 4, 5

enc = HipTileEncoder(0)
keep, batch = [], []
for f in range(N):
    planes = synth_planes_torch(w, h, n_planes=3, seed=9000 + f, device="cuda")
    enc.set_image_u8(planes.permute(1, 2, 0).to(torch.uint8).contiguous())
    enc.encode(3, False, False)
    g = []
    for i, (sx, sy) in enumerate(PASSES):
        bm, rgb = enc.gradient_bitmap(i), enc.gradient_corners(i)
        tb, tr = torch.from_numpy(bm).cuda(), torch.from_numpy(np.concatenate([rgb, np.zeros(16, np.uint8)])).cuda()
        keep += [tb, tr]
        g.append(("g", sx, sy, tb.data_ptr(), bm.size, tr.data_ptr(), rgb.size))
    pix, typ = enc.dynamic_tile_compressor()
    tt, tp = torch.from_numpy(np.concatenate([typ, np.zeros(16, np.uint8)])).cuda(), torch.from_numpy(np.concatenate([pix, np.zeros(16, np.uint8)])).cuda()
    keep += [tt, tp]
    batch.append(g + [("1", tt.data_ptr(), typ.size, tp.data_ptr(), pix.size)])
torch.cuda.synchronize()
enc.close()

rng = np.random.default_rng(N * 100003 + size)
origins = [(int(rng.integers(0, (w - win) // 8 + 1)) * 8, int(rng.integers(0, (h - win) // 8 + 1)) * 8) for _ in range(N)]
# the gather of the whole form: one index per output pixel into the flattened [N * h * w] pixel rows
oy = torch.tensor([o[1] for o in origins], device="cuda").view(N, 1, 1)
ox = torch.tensor([o[0] for o in origins], device="cuda").view(N, 1, 1)
idx = (torch.arange(N, device="cuda").view(N, 1, 1) * h + oy + torch.arange(win, device="cuda").view(1, win, 1)) * w + ox + torch.arange(win, device="cuda").view(1, 1, win)
idx = idx.reshape(-1)

dec, wdec = HipTileDecoder(0), HipTileDecoder(0)                                # a handle per form: each keeps its buffers from one repetition to the next
whole = torch.zeros((N, h, w, 3), dtype=torch.uint8, device="cuda")
out_whole = torch.zeros((N, win, win, 3), dtype=torch.uint8, device="cuda")
out_win = torch.zeros((N, win, win, 3), dtype=torch.uint8, device="cuda")


def run_whole():
    dec.begin_batch(w, h, N)
    dec.decode_batch_streams(batch, sync=False)
    dec.image_batch_device(whole)
    torch.index_select(whole.view(N * h * w, 3), 0, idx, out=out_whole.view(N * win * win, 3))


def run_windows():
    wdec.begin_batch(w, h, N)
    wdec.set_batch_windows(origins, win, win)
    wdec.decode_batch_streams(batch, sync=False)
    wdec.image_batch_windows_device(out_win)


def timed(fn) -> float:
    torch.cuda.synchronize(); dec.synchronize(); wdec.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize(); dec.synchronize(); wdec.synchronize()
    return (time.perf_counter() - t) / (inner * N) * 1e3


forms = [("whole+crop", run_whole)] + ([] if whole_only else [("windows", run_windows)])
for _, fn in forms:                                                              # warm-up: code objects, buffers of both handles
    for _ in range(2):
        timed(fn)
if not whole_only:
    assert torch.equal(out_whole, out_win), "the two forms wrote different pixels"
ms = {name: [] for name, _ in forms}
stages = []
for _ in range(reps):
    for name, fn in forms:
        if name == "windows":
            for st in (ST_GRADIENT, ST_1D, ST_DETILE):
                wdec.stage_ms(st)
        ms[name].append(timed(fn))
        if name == "windows":
            stages.append([wdec.stage_ms(st) for st in (ST_GRADIENT, ST_1D, ST_DETILE)])
tree = "YK_TREE build" if os.environ.get("YK_TREE") else "this build"
for name, _ in forms:
    v = ms[name]
    print(f"{N} x {w}x{h}, windows {win}x{win}, {tree}, {name:10s}: median {statistics.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; "
          f"{reps} repetitions of {inner * N} frames)", flush=True)
if stages:
    med = [statistics.median(s[k][0] / max(s[k][1], 1) for s in stages) for k in range(3)]
    print(f"{N} x {w}x{h}, windows {win}x{win}: window stages per batch: gradient {med[0]:.3f}  1-D {med[1]:.3f}  de-tile {med[2]:.3f} ms;  "
          f"windows / whole+crop = {statistics.median(ms['windows']) / statistics.median(ms['whole+crop']):.3f}", flush=True)
dec.close(); wdec.close()
