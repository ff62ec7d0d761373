"""K windows of one image: the loop of single-window decodes against one prepare + renders, from device-resident streams of one encoded image.
Run from the repository root as
    python profiles/decode_prepared/prepared_vs_loop.py <size> [reps]              e.g. 8192 | 16384

  loop       K x (begin + set_window + decode_streams + image_window_device)                       (yk_decode_set_window)
  prep+loop  begin + prepare, then K x render_window                                                (one launch set per window)
  prep+one   begin + prepare, then ONE render_windows call for the K windows                        (yk_decode_render_windows_device)

for K = 1, 16 and 64 distinct 512 x 512 windows and K = 1 and 16 windows of 2048 x 2048, origins from a fixed seed (multiples of 8, so windows
straddle 64-blocks and may overlap).  All forms read the same streams (encoder_streams: where the encoder left them in HBM) and the script
checks that they produce the same bytes.  A repetition is max(1, 8 / K) passes of a form under a host clock that ends in a device synchronisation, divided by the passes; the
forms alternate after a warm-up of each.  Prints the median, minimum and maximum per repetition (all K windows) over the repetitions, then
for the prepared forms what one call costs alone: prepare (begin + prepare, synchronised), the first render_windows of the K windows, and
the same call again when every block is rendered (the de-tile alone), with the stage intervals of the first render (yk_stage_ms)."""
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

size = int(sys.argv[1])
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
w = h = size
ST = (3, 4, 5)                                                               # gradient, 1-D, de-tile

enc = HipTileEncoder(0)
planes = synth_planes_torch(w, h, n_planes=3, seed=4242, device="cuda")
enc.set_image_u8(planes.permute(1, 2, 0).to(torch.uint8).contiguous())
del planes
enc.encode(3, False, False)
dec = HipTileDecoder(0)
calls = dec.encoder_streams(enc)


def origins_of(k, side):
    rng = np.random.default_rng(1000 * side + k)
    seen = []
    while len(seen) < k:
        o = (int(rng.integers(0, (w - side) // 8 + 1)) * 8, int(rng.integers(0, (h - side) // 8 + 1)) * 8)
        if o not in seen:
            seen.append(o)
    return seen


def run_loop(origins, side, out):
    for k, (x0, y0) in enumerate(origins):
        dec.begin(w, h)
        dec.set_window(x0, y0, side, side)
        dec.decode_streams(calls, sync=False)
        dec.image_window_device(out=out[k])


def run_prep_loop(origins, side, out):
    dec.begin(w, h)
    dec.prepare(calls, sync=False)
    for k, (x0, y0) in enumerate(origins):
        dec.render_window(x0, y0, side, side, out=out[k])


def run_prep_one(origins, side, out):
    dec.begin(w, h)
    dec.prepare(calls, sync=False)
    dec.render_windows(origins, side, side, out=out)


def clock(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    dec.synchronize(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def fmt(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} - {max(v):.3f})"


print(f"# {w} x {h}, {reps} repetitions, forms alternating; a figure is one pass over all K windows", flush=True)
for side, ks in ((512, (1, 16, 64)), (2048, (1, 16))):
    for k in ks:
        origins = origins_of(k, side)
        outs = [torch.empty((k, side, side, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
        forms = [("loop", run_loop, outs[0]), ("prep+loop", run_prep_loop, outs[1]), ("prep+one", run_prep_one, outs[2])]
        for _, fn, out in forms:
            clock(lambda: fn(origins, side, out))                            # warm-up of every shape
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"K = {k}, {side}: the forms differ"
        t = {name: [] for name, _, _ in forms}
        inner = max(1, 8 // k)                                               # passes per clock: a pass over few windows is short
        for _ in range(reps):
            for name, fn, out in forms:
                t[name].append(clock(lambda: fn(origins, side, out), inner))
        print(f"K = {k:2d} windows of {side:4d} x {side:4d}:  " + "   ".join(f"{name} {fmt(v)}" for name, v in t.items()), flush=True)
        prep, first, again, stages = [], [], [], []
        for _ in range(reps):
            prep.append(clock(lambda: (dec.begin(w, h), dec.prepare(calls, sync=False))))
            for st in ST:
                dec.stage_ms(st)
            first.append(clock(lambda: dec.render_windows(origins, side, side, out=outs[2])))
            stages.append([dec.stage_ms(st)[0] for st in ST])
            again.append(clock(lambda: dec.render_windows(origins, side, side, out=outs[2])))
        blocks = dec.prepared_blocks
        med = [statistics.median(s[i] for s in stages) for i in range(3)]
        print(f"      alone: prepare {fmt(prep)}   first render {fmt(first)}   render again {fmt(again)}   blocks {blocks[0]} of {blocks[1]}"
              f"   first render's stages: gradient {med[0]:.3f}  1-D {med[1]:.3f}  de-tile {med[2]:.3f} ms", flush=True)
dec.close(); enc.close()
