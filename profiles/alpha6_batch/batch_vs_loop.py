"""Per-frame time of the 6-bit mask mode 'ALPM' values (ProcessAlpha(false)) of N equally shaped RGBA frames: ONE yk_alpha_values_mask_batch
call against a loop of single-image calls on a second handle, the only way the parent commit offers.  Run from the repository root as
    python profiles/alpha6_batch/batch_vs_loop.py <frames> <size> [reps] [--profile]      e.g. 256 512 | 64 2048 | 4 4096

Every frame has YAIK-synth v1 colour planes and analog alpha (1..254) in a box of about 0.7 of each side with 0 around it; about one tile in
eight inside the box is rejected (all zero), another pattern per frame.

  loop         per frame, single-image handle: set_image + alpha_reject + alpha_finish + alpha_values(False), payload copied to the host
  loop_values  the alpha_values(False) calls of that loop alone (a host clock around each call, which ends in a synchronisation)
  batch        alpha_values_mask_batch() behind encode_batch: every payload copied to the host, like the loop's
  batch_dev    alpha_mask_payloads_device(): the payloads stay in HBM

The batch handle's alpha stage (encode_batch) runs once, outside the clock; the loop cannot leave its own out, since set_image drops it, which is
why loop_values is printed beside it.  The script checks that loop and batch produce the same modes, boxes and bytes.  A repetition is `inner`
passes over the N frames (at least 64 frames) under a host clock that ends in a device synchronisation; the forms alternate after a warm-up of
each.  Prints per-frame median, minimum, maximum.  --profile runs each batch form once, untimed (for rocprofv3)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

args = [a for a in sys.argv[1:] if not a.startswith("--")]
profile = "--profile" in sys.argv
N, size = int(args[0]), int(args[1])
reps = int(args[2]) if len(args) > 2 else 7
w = h = size
inner = max(1, -(-64 // N))

# ---- the frames: [N, 4, h, w] int32 on the device -------------------------------------------------------------------------------------------------
bx, by, bw, bh = (w // 8) & ~15, (h // 8) & ~15, int(w * 0.7) & ~15, int(h * 0.7) & ~15
frames = torch.zeros((N, 4, h, w), dtype=torch.int32, device="cuda")
gen = torch.Generator(device="cuda").manual_seed(6)
for f in range(N):
    frames[f, :3] = synth_planes_torch(w, h, n_planes=3, seed=9000 + (f % 8), device="cuda")
    a = torch.randint(1, 255, (bh, bw), generator=gen, device="cuda", dtype=torch.int32)
    keep = torch.rand((bh // 16, bw // 16), generator=gen, device="cuda") >= 0.125
    keep[0, :] = keep[-1, :] = True                                              # the box of kept tiles stays the box
    keep[:, 0] = keep[:, -1] = True
    frames[f, 3, by:by + bh, bx:bx + bw] = a * keep.repeat_interleave(16, 0).repeat_interleave(16, 1)
torch.cuda.synchronize()

one = HipTileEncoder(0)
loop_out = [None] * N
values_s = [0.0]


def enc_loop():
    for f in range(N):
        one.set_image(frames[f])
        one.alpha_reject()
        one.alpha_finish(None)
        t = time.perf_counter()
        loop_out[f] = one.alpha_values(False)
        values_s[0] += time.perf_counter() - t


benc = HipTileEncoder(0)
benc.set_batch(frames)
benc.encode_batch()
benc.synchronize()
batch_out, dev_out = [None], [None]


def enc_batch():
    batch_out[0] = benc.alpha_values_mask_batch()


def enc_batch_dev():
    dev_out[0] = benc.alpha_mask_payloads_device()


forms = [("loop", enc_loop), ("batch", enc_batch), ("batch_dev", enc_batch_dev)]
handles = [one, benc]


def fence():
    torch.cuda.synchronize()
    for x in handles:
        x.synchronize()


def timed(fn) -> float:
    fence()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    fence()
    return (time.perf_counter() - t) / (inner * N) * 1e3


if profile:
    enc_batch(); enc_batch_dev()
    fence()
    sys.exit(0)
for _, fn in forms:                                                              # warm-up: code objects, buffers of every handle
    for _ in range(2):
        timed(fn)
ms = {name: [] for name, _ in forms}
ms["loop_values"] = []
for _ in range(reps):
    for name, fn in forms:
        values_s[0] = 0.0
        ms[name].append(timed(fn))
        if name == "loop":
            ms["loop_values"].append(values_s[0] / (inner * N) * 1e3)
enc_loop(); enc_batch(); enc_batch_dev(); benc.synchronize()
rejected = 0
for f in range(N):
    a, b, d = loop_out[f], batch_out[0][f], dev_out[0][f]
    assert a["mode"] == b["mode"] == d[0] == 3 and a["bbox"] == b["bbox"] == d[1] and np.array_equal(a["payload"], b["payload"]), f"frame {f} differs"
    rejected += a["payload"].size < a["bbox"][2] // 4 * 3 * a["bbox"][3]
    got = torch.empty(d[3], dtype=torch.uint8, device="cuda")
    rc = benc._L.yk_device_copy(benc._h, got.data_ptr(), d[2], d[3])
    benc.synchronize()
    assert rc == 0 and np.array_equal(got.cpu().numpy(), a["payload"]), f"frame {f}'s device payload differs"
assert rejected == N, "every frame has rejected tiles inside its box"
print(f"{N} x {w}x{h} RGBA: loop and batch payloads are byte-identical (mode 3, rejected tiles inside every box)", flush=True)
for name in ("loop", "loop_values", "batch", "batch_dev"):
    v = ms[name]
    print(f"{N} x {w}x{h} RGBA, {name:11s}: median {statistics.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; "
          f"{reps} repetitions of {inner * N} frames)", flush=True)
print(f"{N} x {w}x{h} RGBA: batch median {'<' if statistics.median(ms['batch']) < min(ms['loop']) else '>='} loop minimum; "
      f"batch / loop = {statistics.median(ms['batch']) / statistics.median(ms['loop']):.3f}, "
      f"batch / loop_values = {statistics.median(ms['batch']) / statistics.median(ms['loop_values']):.3f}", flush=True)
for x in handles:
    x.close()
