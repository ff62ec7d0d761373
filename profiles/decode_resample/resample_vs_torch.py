"""Per-frame rectangles resampled to one size by the decoder, against the route a caller had before: decode every frame whole, write
uint8 [N, H, W, 3], and then per frame in torch slice, .float(), F.interpolate(bilinear, antialias=False), scale and bias, flip, and store into the
stacked result.  From device-resident streams of N encoded frames; run from the repository root as
    python profiles/decode_resample/resample_vs_torch.py <frames> <size> <out> <float16|bfloat16|float32> <crop|whole|identity> [reps]
                                                     e.g. 256 512 224 float16 crop | 64 2048 512 float16 crop | 1 8192 1024 float16 whole

  crop      rectangles from random_resized_crop_rects(seed=0), every second frame mirrored, ImageNet statistics, CHW output:
              torch      begin_batch + the chunks (whole frames) + image_batch_device + the per-frame torch loop
              resampled  begin_batch + set_batch_rects + the chunks (each frame's cover) + image_resampled_batch_device
  whole     the same with every rectangle the whole frame (one frame: the single-image calls and image_resampled_device)
  identity  what the gather costs over the de-tile: out x out pixel windows at the rectangles' origins,
              norm       set_batch_windows(px=True) + the chunks + image_norm_batch_device
              resampled  set_batch_rects of the same rectangles + the chunks + image_resampled_batch_device((out, out))

A repetition is `inner` calls (at least 256 frames, at least 16 calls for one frame) under a host clock that ends in a device synchronisation; the
forms alternate after a warm-up of each.  Prints per-frame median, minimum and maximum over the repetitions, the ratio with the baseline's spread,
the largest difference between the two results in units of one grey level, and each form's de-tile interval per call."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import torch.nn.functional as F

from yaik_amd.augment import random_resized_crop_rects
from yaik_amd.decoder import HipTileDecoder, norm_params
from yaik_amd.encoder import PASSES, HipTileEncoder
from yaik_amd.synth import synth_planes_torch

N, size, out_size, dtype_name, mode = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
reps = int(sys.argv[6]) if len(sys.argv) > 6 else 7
dtype = getattr(torch, dtype_name)
w = h = size
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

if mode == "whole":
    rects = np.array([(0, 0, w, h)] * N, np.int32)
else:
    rects = random_resized_crop_rects(N, w, h, seed=0)
    if mode == "identity":                                                    # the same origins, every rectangle out x out (pulled back inside the image)
        rects[:, 2:] = out_size
        rects[:, 0] = np.minimum(rects[:, 0], w - out_size)
        rects[:, 1] = np.minimum(rects[:, 1], h - out_size)
flags = [f % 2 == 1 for f in range(N)]
scale, bias = norm_params([0.485 * 255, 0.456 * 255, 0.406 * 255], [0.229 * 255, 0.224 * 255, 0.225 * 255])
t_scale, t_bias = torch.from_numpy(scale[:3]).cuda().view(1, 3, 1, 1), torch.from_numpy(bias[:3]).cuda().view(1, 3, 1, 1)

base = "norm" if mode == "identity" else "torch"
decs = {name: HipTileDecoder(0) for name in (base, "resampled")}              # a handle per form: each keeps its buffers
u8 = torch.zeros((N, h, w, 3), dtype=torch.uint8, device="cuda") if mode != "identity" else None
outs = {name: torch.zeros((N, 3, out_size, out_size), dtype=dtype, device="cuda") for name in decs}
single = N == 1 and mode == "whole"


def run_torch():
    d = decs["torch"]
    if single:
        d.begin(w, h)
        d.decode_streams(batch[0], sync=False)
        d.image_device(u8[0])
    else:
        d.begin_batch(w, h, N)
        d.decode_batch_streams(batch, sync=False)
        d.image_batch_device(u8)
    o = outs["torch"]
    for f in range(N):
        x0, y0, sw, sh = (int(v) for v in rects[f])
        t = u8[f, y0:y0 + sh, x0:x0 + sw].permute(2, 0, 1)[None].float()
        t = F.interpolate(t, size=(out_size, out_size), mode="bilinear", align_corners=False, antialias=False) * t_scale + t_bias
        o[f] = (t.flip(-1) if flags[f] else t)[0]


def run_norm():
    d = decs["norm"]
    d.begin_batch(w, h, N)
    d.set_batch_windows(rects[:, :2].copy(), out_size, out_size, px=True)
    d.decode_batch_streams(batch, sync=False)
    d.image_norm_batch_device(dtype, scale=scale, bias=bias, mirror=flags, out=outs["norm"], channels=3, planar=True)


def run_resampled():
    d = decs["resampled"]
    if single:
        d.begin(w, h)
        d.decode_streams(batch[0], sync=False)
        d.image_resampled_device((out_size, out_size), dtype=dtype, scale=scale, bias=bias, mirror=flags[0], out=outs["resampled"][0], channels=3, planar=True)
        return
    d.begin_batch(w, h, N)
    if mode != "whole":
        d.set_batch_rects(rects)
    d.decode_batch_streams(batch, sync=False)
    d.image_resampled_batch_device((out_size, out_size), dtype=dtype, scale=scale, bias=bias, mirror=flags, out=outs["resampled"], channels=3, planar=True)


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


forms = [(base, run_norm if mode == "identity" else run_torch), ("resampled", run_resampled)]
for _, fn in forms:
    for _ in range(2):
        timed(fn)
grey = float(((outs[base].float() - outs["resampled"].float()).abs() / t_scale.abs()).max())
ms = {name: [] for name, _ in forms}
detile = {name: [] for name, _ in forms}
for _ in range(reps):
    for name, fn in forms:
        decs[name].stage_ms(ST_DETILE)
        ms[name].append(timed(fn))
        t, calls = decs[name].stage_ms(ST_DETILE)
        detile[name].append(t / max(calls, 1))
tag = f"{N} x {w}x{h} -> {out_size}x{out_size}, {mode}, {dtype_name} chw"
for name, _ in forms:
    v = ms[name]
    print(f"{tag}, {name:9s}: median {statistics.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; {reps} repetitions of {inner * N} frames); "
          f"de-tile {statistics.median(detile[name]) * 1e3:.1f} us per call", flush=True)
c, p = statistics.median(ms[base]), statistics.median(ms["resampled"])
print(f"{tag}: resampled / {base} = {p / c:.3f}; resampled - {base} = {p - c:+.4f} ms per frame, {base}'s own min-max spread "
      f"{max(ms[base]) - min(ms[base]):.4f}; largest difference {grey:.3f} grey levels", flush=True)
for d in decs.values():
    d.close()
