"""A reduced image two ways, from device-resident encoder streams.  Run from the repository root as
    python profiles/decode_scaled/scaled_vs_full.py image <size> [reps]            e.g. 8192 | 16384
    python profiles/decode_scaled/scaled_vs_full.py batch <frames> <size> [reps]   e.g. 256 512

  (a) full+torch  the whole decode + image_device (image_batch_device) + the integer box reduction in torch: the full-size pixels are written
                  and read back by a second pass (the reduction sums int16 copies of the pixels in int32; the full-size tensor is allocated once,
                  outside the clock)
  (b) scaled      the same decode + image_scaled_device (image_scaled_batch_device): the de-tile kernel writes the reduced pixels only

for level 1, 2 and 3.  Both forms read the same streams and the script checks that they produce the same bytes.  A repetition is one pass of a form
under a host clock that ends in a device synchronisation; the forms alternate after a warm-up of each.  Prints the median, minimum and maximum over
the repetitions, and beside them the YK_STAGE_DEC_DETILE interval (yk_stage_ms) of the scaled and of the full-size output of the same decode."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

mode = sys.argv[1]
if mode == "batch":
    frames, size = int(sys.argv[2]), int(sys.argv[3])
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
else:
    frames, size = 0, int(sys.argv[2])
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
w = h = size
DETILE = 5

enc = HipTileEncoder(0)
dec = HipTileDecoder(0)
if frames:
    u8 = torch.stack([synth_planes_torch(w, h, n_planes=3, seed=4242 + f, device="cuda").permute(1, 2, 0).to(torch.uint8) for f in range(frames)]).contiguous()
    enc.set_batch_u8(u8)
    del u8
    enc.encode_batch(3, False)
    dec.begin_batch(w, h, frames)                                            # encoder_batch_streams checks the shapes against the batch begun
    streams = dec.encoder_batch_streams(enc)
    full = torch.empty((frames, h, w, 3), dtype=torch.uint8, device="cuda")
else:
    planes = synth_planes_torch(w, h, n_planes=3, seed=4242, device="cuda")
    enc.set_image_u8(planes.permute(1, 2, 0).to(torch.uint8).contiguous())
    del planes
    enc.encode(3, False, False)
    streams = dec.encoder_streams(enc)
    full = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")


def decode():
    if frames:
        dec.begin_batch(w, h, frames)
        dec.decode_batch_streams(streams, sync=False)
    else:
        dec.begin(w, h)
        dec.decode_streams(streams, sync=False)


def torch_reduce(t, level):
    s = 1 << level
    hh, ww, c = t.shape[-3:]
    v = t.reshape(t.shape[:-3] + (hh // s, s, ww // s, s, c)).to(torch.int16).sum(dim=(-2, -4), dtype=torch.int32)
    return ((v + (s * s) // 2) >> (2 * level)).to(torch.uint8)


def run_full(level):
    decode()
    if frames:
        dec.image_batch_device(out=full)
    else:
        dec.image_device(out=full)
    return torch_reduce(full, level)


def run_scaled(level, out):
    decode()
    if frames:
        dec.image_scaled_batch_device(level, out=out)
    else:
        dec.image_scaled_device(level, out=out)
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    dec.synchronize(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fmt(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} - {max(v):.3f})"


what = f"{frames} x {w} x {h}" if frames else f"{w} x {h}"
print(f"# {what}, {reps} repetitions, forms alternating; a figure is decode + output (+ reduction)", flush=True)
for level in (1, 2, 3):
    shape = ((frames,) if frames else ()) + (h >> level, w >> level, 3)
    out = torch.empty(shape, dtype=torch.uint8, device="cuda")
    a = run_full(level)
    b = run_scaled(level, out)
    torch.cuda.synchronize()
    assert torch.equal(a, b), f"level {level}: the forms differ"
    del a
    t = {"full+torch": [], "scaled": []}
    dt = {"full": [], "scaled": []}
    for _ in range(reps):
        dec.stage_ms(DETILE)
        t["full+torch"].append(clock(lambda: run_full(level)))
        dt["full"].append(dec.stage_ms(DETILE)[0])
        t["scaled"].append(clock(lambda: run_scaled(level, out)))
        dt["scaled"].append(dec.stage_ms(DETILE)[0])
    print(f"level {level} ({shape[-2]} x {shape[-3]}):  (a) full+torch {fmt(t['full+torch'])}   (b) scaled {fmt(t['scaled'])}   "
          f"de-tile interval: full {fmt(dt['full'])}   scaled {fmt(dt['scaled'])}", flush=True)
dec.close(); enc.close()
