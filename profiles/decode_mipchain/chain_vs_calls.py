"""A whole mip chain two ways, from device-resident encoder streams.  Run from the repository root as
    python profiles/decode_mipchain/chain_vs_calls.py image <size> [reps]            e.g. 8192 | 16384
    python profiles/decode_mipchain/chain_vs_calls.py batch <frames> <size> [reps]   e.g. 256 512

  (a) calls  what the library offered before the chain call: the decode, image_device, image_scaled_device at levels 1, 2 and 3, then the levels
             from 4 up as integer box sums in torch from the full-size tensor (int64 sums of 16 x 16 boxes, folded 2 x 2 per level, rounded once
             per level from the exact sum): nothing else gives the same function
  (b) chain  the same decode, then one image_mipchain_device (image_mipchain_batch_device)

Both forms read the same streams and the script checks that they produce the same bytes at every level.  A repetition is one pass of a form under
a host clock that ends in a device synchronisation; the forms alternate after a warm-up of each.  Prints the median, minimum and maximum over the
repetitions, and beside them the YK_STAGE_DEC_DETILE figures (yk_stage_ms): the sum of the intervals of the four calls of (a), the interval of
the full-size call alone, and the interval of the one chain call."""
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
lead = (frames,) if frames else ()

enc = HipTileEncoder(0)
dec = HipTileDecoder(0)
if frames:
    u8 = torch.stack([synth_planes_torch(w, h, n_planes=3, seed=4242 + f, device="cuda").permute(1, 2, 0).to(torch.uint8) for f in range(frames)]).contiguous()
    enc.set_batch_u8(u8)
    del u8
    enc.encode_batch(3, False)
    dec.begin_batch(w, h, frames)                                            # encoder_batch_streams checks the shapes against the batch begun
    streams = dec.encoder_batch_streams(enc)
else:
    planes = synth_planes_torch(w, h, n_planes=3, seed=4242, device="cuda")
    enc.set_image_u8(planes.permute(1, 2, 0).to(torch.uint8).contiguous())
    del planes
    enc.encode(3, False, False)
    streams = dec.encoder_streams(enc)
top = min(w, h).bit_length() - 1
outs = {form: [torch.empty(lead + (h >> k, w >> k, 3), dtype=torch.uint8, device="cuda") for k in range(top + 1)] for form in ("calls", "chain")}


def decode():
    if frames:
        dec.begin_batch(w, h, frames)
        dec.decode_batch_streams(streams, sync=False)
    else:
        dec.begin(w, h)
        dec.decode_streams(streams, sync=False)


def run_calls():
    o = outs["calls"]
    decode()
    if frames:
        dec.image_batch_device(out=o[0])
        for k in (1, 2, 3):
            dec.image_scaled_batch_device(k, out=o[k])
    else:
        dec.image_device(out=o[0])
        for k in (1, 2, 3):
            dec.image_scaled_device(k, out=o[k])
    full = o[0]
    hh, ww = h >> 4 << 4, w >> 4 << 4
    v = full[..., :hh, :ww, :].reshape(lead + (hh // 16, 16, ww // 16, 16, 3)).sum(dim=(-2, -4), dtype=torch.int64)
    for k in range(4, top + 1):
        if k > 4:
            hh, ww = v.shape[-3] >> 1 << 1, v.shape[-2] >> 1 << 1
            v = v[..., :hh, :ww, :].reshape(lead + (hh // 2, 2, ww // 2, 2, 3)).sum(dim=(-2, -4))
        o[k].copy_(((v + (1 << (2 * k - 1))) >> (2 * k)).to(torch.uint8))


def run_chain():
    decode()
    if frames:
        dec.image_mipchain_batch_device(out=outs["chain"])
    else:
        dec.image_mipchain_device(out=outs["chain"])


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    dec.synchronize(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fmt(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} - {max(v):.3f})"


what = f"{frames} x {w} x {h}" if frames else f"{w} x {h}"
print(f"# {what}, levels 0..{top}, {reps} repetitions, forms alternating; a figure is decode + every level of the chain", flush=True)
run_calls(); run_chain()
torch.cuda.synchronize()
for k in range(top + 1):
    assert torch.equal(outs["calls"][k], outs["chain"][k]), f"level {k}: the forms differ"
t = {"calls": [], "chain": []}
dt = {"four": [], "full": [], "chain": []}
for _ in range(reps):
    dec.synchronize(); dec.stage_ms(DETILE)
    t["calls"].append(clock(run_calls))
    four = dec.stage_ms(DETILE)
    t["chain"].append(clock(run_chain))
    one = dec.stage_ms(DETILE)
    dt["four"].append(four[0]); dt["chain"].append(one[0])
    assert four[1] == 4 and one[1] == 1, (four, one)
# the full-size call alone, for the same decode
for _ in range(reps):
    decode()
    dec.synchronize(); dec.stage_ms(DETILE)
    (dec.image_batch_device if frames else dec.image_device)(out=outs["calls"][0])
    dec.synchronize()
    dt["full"].append(dec.stage_ms(DETILE)[0])
print(f"(a) calls {fmt(t['calls'])}   (b) chain {fmt(t['chain'])}", flush=True)
print(f"de-tile intervals: the four calls of (a) together {fmt(dt['four'])}   the full-size call alone {fmt(dt['full'])}   the chain call {fmt(dt['chain'])}", flush=True)
dec.close(); enc.close()
