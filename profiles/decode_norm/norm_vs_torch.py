"""Normalised, mirrored pixel windows written by the de-tile kernel, against the route a caller had before: the uint8 pixel-window call and then
torch -- .to(dtype), the affine step, a flip of the flagged frames, and .contiguous() in the layout asked for.  From device-resident streams of N
encoded frames; run from the repository root as
    python profiles/decode_norm/norm_vs_torch.py <frames> <size> <window> <float16|bfloat16|float32> <chw|hwc> [reps]
                                                                         e.g. 256 512 224 float16 chw | 64 2048 512 float32 hwc | 1 8192 512 float16 chw

  uint8+torch  set_[batch_]window[s](px=True) + the chunks + image_[batch_]window[s]_device (uint8) + .to(dtype) * scale + bias, flip, permute, contiguous
  norm         set_[batch_]window[s](px=True) + the chunks + image_norm[_batch]_device                 (yk_decode_output_norm[_batch]_device)

One frame is the single-image calls, more are the batch calls.  Every origin is (+3, +5) from a random 8-aligned one (fixed seed); every second frame
is mirrored; scale and bias are norm_params of the ImageNet means and stds x 255.  The torch route rounds after every step in `dtype`, so the two
agree bit for bit in float32 only; the script prints whether they do (the GPU tests hold the new call to its own contract).  A repetition is `inner`
calls (at least 256 frames, at least 16 calls) under a host clock that ends in a device synchronisation; the forms alternate after a warm-up of
each.  Prints per-frame median, minimum and maximum over the repetitions, the ratio, and the de-tile interval per call."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from yaik_amd.decoder import HipTileDecoder, norm_params
from yaik_amd.encoder import PASSES, HipTileEncoder
from yaik_amd.synth import synth_planes_torch

N, size, win, dtype_name, layout = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
reps = int(sys.argv[6]) if len(sys.argv) > 6 else 7
dtype, planar = getattr(torch, dtype_name), layout == "chw"
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

rng = np.random.default_rng(N * 100003 + size)
cov = (win + max(DX, DY) + 7) // 8 * 8
origins = [(int(rng.integers(0, (w - cov) // 8 + 1)) * 8 + DX, int(rng.integers(0, (h - cov) // 8 + 1)) * 8 + DY) for _ in range(N)]
flags = [f % 2 == 1 for f in range(N)] if N > 1 else [True]
scale, bias = norm_params([0.485 * 255, 0.456 * 255, 0.406 * 255], [0.229 * 255, 0.224 * 255, 0.225 * 255])
t_scale, t_bias = torch.from_numpy(scale[:3]).cuda().to(dtype), torch.from_numpy(bias[:3]).cuda().to(dtype)
t_flags = torch.tensor(flags, device="cuda")

decs = {name: HipTileDecoder(0) for name in ("uint8+torch", "norm")}             # a handle per form: each keeps its buffers
lead = (N,) if N > 1 else ()
u8 = torch.zeros(lead + (win, win, 3), dtype=torch.uint8, device="cuda")
shape = lead + ((3, win, win) if planar else (win, win, 3))
outs = {name: torch.zeros(shape, dtype=dtype, device="cuda") for name in decs}


def decode(d):
    if N == 1:
        d.begin(w, h)
        d.set_window(origins[0][0], origins[0][1], win, win, px=True)
        d.decode_streams(batch[0], sync=False)
    else:
        d.begin_batch(w, h, N)
        d.set_batch_windows(origins, win, win, px=True)
        d.decode_batch_streams(batch, sync=False)


def run_torch():
    d = decs["uint8+torch"]
    decode(d)
    if N == 1:
        d.image_window_device(u8)
    else:
        d.image_batch_windows_device(u8)
    t = u8.to(dtype) * t_scale + t_bias                                          # HWC: the channel is the last axis
    if N == 1:
        t = t.flip(-2) if flags[0] else t
    else:
        t = torch.where(t_flags.view(-1, 1, 1, 1), t.flip(-2), t)
    outs["uint8+torch"].copy_(t.movedim(-1, -3) if planar else t)                # the .contiguous() of the result, into a buffer kept like the other's


def run_norm():
    d = decs["norm"]
    decode(d)
    if N == 1:
        d.image_norm_device(dtype, scale=scale, bias=bias, mirror=flags[0], out=outs["norm"], channels=3, planar=planar)
    else:
        d.image_norm_batch_device(dtype, scale=scale, bias=bias, mirror=flags, out=outs["norm"], channels=3, planar=planar)


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


forms = [("uint8+torch", run_torch), ("norm", run_norm)]
for _, fn in forms:
    for _ in range(2):
        timed(fn)
same = torch.equal(outs["uint8+torch"].view(torch.int32 if dtype == torch.float32 else torch.int16), outs["norm"].view(torch.int32 if dtype == torch.float32 else torch.int16))
close = torch.allclose(outs["uint8+torch"].float(), outs["norm"].float(), rtol=2.0 ** -6, atol=2.0 ** -6)
ms = {name: [] for name, _ in forms}
detile = {name: [] for name, _ in forms}
for _ in range(reps):
    for name, fn in forms:
        decs[name].stage_ms(ST_DETILE)
        ms[name].append(timed(fn))
        t, calls = decs[name].stage_ms(ST_DETILE)
        detile[name].append(t / max(calls, 1))
tag = f"{N} x {w}x{h}, windows {win}x{win} at (+{DX}, +{DY}), {dtype_name} {layout}"
for name, _ in forms:
    v = ms[name]
    print(f"{tag}, {name:11s}: median {statistics.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; {reps} repetitions of {inner * N} frames); "
          f"de-tile {statistics.median(detile[name]) * 1e3:.1f} us per call", flush=True)
c, p = statistics.median(ms["uint8+torch"]), statistics.median(ms["norm"])
print(f"{tag}: norm / uint8+torch = {p / c:.3f}; norm - uint8+torch = {p - c:+.4f} ms per frame, uint8+torch's own min-max spread "
      f"{max(ms['uint8+torch']) - min(ms['uint8+torch']):.4f}; same bits {same}, close {close}", flush=True)
for d in decs.values():
    d.close()
