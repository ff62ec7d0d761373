"""A window at a pixel offset, cropped in the de-tile, against the route a caller had before: decode the window's 8-aligned cover with the aligned
call and slice it in torch.  From device-resident streams of N encoded frames; run from the repository root as
    python profiles/decode_window_px/px_vs_cover.py <frames> <size> <window> [reps]          e.g. 1 8192 512 | 64 2048 512 | 256 512 224

  cover+slice  set_[batch_]window[s](cover) + the chunks + image_[batch_]window[s]_device + out[..., 5:5 + wh, 3:3 + ww, :].contiguous()
  px           set_[batch_]window[s](px=True) + the chunks + image_[batch_]window[s]_device          (yk_decode_set_window_px / _batch_windows_px)
  aligned      the px form's rectangle moved to its aligned origin: the existing kernels, what clipping costs on top of them

One frame is the single-image calls (begin, set_window, decode_streams), more are the batch calls.  Every origin is (+3, +5) from a random
8-aligned one (fixed seed), so every window is cut by its cover on all four sides.  The script checks that cover+slice and px write the same
bytes.  A repetition is `inner` calls (at least 256 frames, at least 16 calls) under a host clock that ends in a device synchronisation; the
forms alternate after a warm-up of each.  Prints per-frame median, minimum and maximum over the repetitions and the de-tile interval per call."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import PASSES, HipTileEncoder
from yaik_amd.synth import synth_planes_torch

N, size, win = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
w = h = size
DX, DY = 3, 5
inner = max(16 if N == 1 else 1, -(-256 // N))
ST_DETILE = 5

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

cov = (win + DX + 7) // 8 * 8                                                    # the cover of a window at (+3, +5) from an aligned origin: one size
assert cov == (win + DY + 7) // 8 * 8 and cov <= size
rng = np.random.default_rng(N * 100003 + size)
base = [(int(rng.integers(0, (w - cov) // 8 + 1)) * 8, int(rng.integers(0, (h - cov) // 8 + 1)) * 8) for _ in range(N)]
origins = [(x + DX, y + DY) for x, y in base]

decs = {name: HipTileDecoder(0) for name in ("cover+slice", "px", "aligned")}   # a handle per form: each keeps its buffers
lead = (N,) if N > 1 else ()
cover_out = torch.zeros(lead + (cov, cov, 3), dtype=torch.uint8, device="cuda")
outs = {name: torch.zeros(lead + (win, win, 3), dtype=torch.uint8, device="cuda") for name in decs}


def decode(d, rects, ww, px):
    if N == 1:
        d.begin(w, h)
        d.set_window(rects[0][0], rects[0][1], ww, ww, px=px)
        d.decode_streams(batch[0], sync=False)
    else:
        d.begin_batch(w, h, N)
        d.set_batch_windows(rects, ww, ww, px=px)
        d.decode_batch_streams(batch, sync=False)


def output(d, out):
    return d.image_window_device(out) if N == 1 else d.image_batch_windows_device(out)


def run_cover():
    d = decs["cover+slice"]
    decode(d, base, cov, False)
    output(d, cover_out)
    outs["cover+slice"].copy_(cover_out[..., DY:DY + win, DX:DX + win, :])      # the .contiguous() of the slice, into a buffer kept like the others'


def run_px():
    decode(decs["px"], origins, win, True)
    output(decs["px"], outs["px"])


def run_aligned():
    decode(decs["aligned"], base, win, False)
    output(decs["aligned"], outs["aligned"])


def fence():
    torch.cuda.synchronize()
    for d in decs.values():
        d.synchronize()


def timed(fn) -> float:
    fence()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    fence()
    return (time.perf_counter() - t) / (inner * N) * 1e3


forms = [("cover+slice", run_cover), ("px", run_px), ("aligned", run_aligned)]
for _, fn in forms:
    for _ in range(2):
        timed(fn)
assert torch.equal(outs["cover+slice"], outs["px"]), "cover+slice and px wrote different pixels"
ms = {name: [] for name, _ in forms}
detile = {name: [] for name, _ in forms}
for _ in range(reps):
    for name, fn in forms:
        decs[name].stage_ms(ST_DETILE)
        ms[name].append(timed(fn))
        t, calls = decs[name].stage_ms(ST_DETILE)
        detile[name].append(t / max(calls, 1))
for name, _ in forms:
    v = ms[name]
    print(f"{N} x {w}x{h}, windows {win}x{win} at (+{DX}, +{DY}), {name:11s}: median {statistics.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; "
          f"{reps} repetitions of {inner * N} frames); de-tile {statistics.median(detile[name]) * 1e3:.1f} us per call", flush=True)
c, p, a = (statistics.median(ms[k]) for k in ("cover+slice", "px", "aligned"))
spread = max(ms["cover+slice"]) - min(ms["cover+slice"])
print(f"{N} x {w}x{h}, windows {win}x{win}: px / cover+slice = {p / c:.3f}, px / aligned = {p / a:.3f}; px - cover+slice = {p - c:+.4f} ms per frame, "
      f"cover+slice's own min-max spread {spread:.4f}", flush=True)
for d in decs.values():
    d.close()
