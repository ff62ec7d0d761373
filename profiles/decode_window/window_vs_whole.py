"""Window decode against whole decode + crop, from device-resident streams of one encoded image.  Run from the repository root as
    python profiles/decode_window/window_vs_whole.py <size> [reps] [--whole-only]              e.g. 8192 | 16384

  whole   begin + decode_streams + image_device + a torch copy of the window's slice into a contiguous tensor      (what a caller did before)
  window  begin + set_window + decode_streams + image_window_device                                                 (yk_decode_set_window)

for windows of 512 x 512, 2048 x 2048 (both centred on a 64-pixel boundary + 8, so they straddle blocks) and the whole image.  Both forms read
the same streams (encoder_streams: where the encoder left them in HBM) and the script checks that they produce the same bytes.  A repetition
is `inner` decodes under a host clock that ends in a device synchronisation; the two forms alternate after a warm-up of each.  Prints the
median, minimum and maximum per decode over the repetitions, and for the window form the stage intervals (gradient, 1-D, de-tile: yk_stage_ms)
per decode, which show the map-sized share that stays.

--whole-only times the whole form alone: it uses nothing this change added, so with YK_TREE=<a checkout of the parent commit, built> the same
script times the parent's path on the same machine in the same visit."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("YK_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

args = [a for a in sys.argv[1:] if not a.startswith("--")]
whole_only = "--whole-only" in sys.argv
size = int(args[0])
reps = int(args[1]) if len(args) > 1 else 7
w = h = size
inner = 8 if size <= 8192 else 3
ST_GRADIENT, ST_1D, ST_DETILE = 3, 4, 5

enc = HipTileEncoder(0)
planes = synth_planes_torch(w, h, n_planes=3, seed=4242, device="cuda")
enc.set_image_u8(planes.permute(1, 2, 0).to(torch.uint8).contiguous())
del planes
enc.encode(3, False, False)
dec = HipTileDecoder(0)
calls = dec.encoder_streams(enc)


def window_of(side):
    if side >= size:
        return (0, 0, w, h)
    o = (size // 2 // 64) * 64 + 8 - side // 2
    return (o, o, side, side)


def run_whole(win, out):
    x0, y0, ww, wh = win
    dec.begin(w, h)
    dec.decode_streams(calls, sync=False)
    img = dec.image_device()
    out.copy_(img[y0:y0 + wh, x0:x0 + ww])


def run_window(win, out):
    dec.begin(w, h)
    dec.set_window(*win)
    dec.decode_streams(calls, sync=False)
    dec.image_window_device(out=out)


def timed(fn, win, out):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn(win, out)
    dec.synchronize(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def fmt(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} - {max(v):.3f})"


print(f"# {w} x {h}, {reps} repetitions of {inner} decodes, forms alternating" + (" [whole form only]" if whole_only else ""))
for side in (512, 2048, size):
    win = window_of(side)
    a = torch.empty((win[3], win[2], 3), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    forms = [("whole+crop", run_whole, a)] + ([] if whole_only else [("window", run_window, b)])
    for _, fn, out in forms:
        timed(fn, win, out)                                                  # warm-up of every shape
    if not whole_only:
        assert torch.equal(a, b), f"window {win}: the two forms differ"
    t = {name: [] for name, _, _ in forms}
    stages = []
    for _ in range(reps):
        for name, fn, out in forms:
            if name == "window":
                for st in (ST_GRADIENT, ST_1D, ST_DETILE):
                    dec.stage_ms(st)
            t[name].append(timed(fn, win, out))
            if name == "window":
                stages.append([dec.stage_ms(st) for st in (ST_GRADIENT, ST_1D, ST_DETILE)])
    line = f"window {win[2]:5d} x {win[3]:5d} at ({win[0]}, {win[1]}):  " + "   ".join(f"{name} {fmt(v)}" for name, v in t.items())
    if stages:
        med = [statistics.median(s[k][0] / max(s[k][1], 1) for s in stages) for k in range(3)]
        line += f"   window stages per decode: gradient {med[0]:.3f}  1-D {med[1]:.3f}  de-tile {med[2]:.3f} ms"
    print(line, flush=True)
dec.close(); enc.close()
