"""Per-frame time of the 'ALPM' alpha values of N equally shaped RGBA frames: ONE batch call against a loop of single-image calls, for the
encode side and the decode side.  Run from the repository root as
    python profiles/alpha_batch/batch_vs_loop.py <frames> <size> [reps] [--loop-only] [--profile]      e.g. 256 512 | 64 2048 | 2 8192

Every frame has analog alpha (1..254) in a box of about half the frame and 0 around it.

encode (planes bound in place; the loop is the only way the parent commit offers)
  loop        per frame, single-image handle: set_image + mip_prefilter + alpha_values(True)
  loop_lean   the same without mip_prefilter's result fetch: set_image + alpha_reject + alpha_finish + alpha_values(True)
  batch       alpha_values_batch() after encode_batch: payloads copied to the host, like the loop's
  batch_dev   alpha_payloads_device(): the payloads stay in HBM
decode (host payloads, as yk_decode_alpha takes them; [N, H, W, 4] out)
  loop        per frame: begin + decompress_alpha(to_host=False) + image_device(alpha=-1) into out[f]
  batch       begin_batch + decompress_alpha_batch(host arrays) + image_batch_device(alpha_from_planes=True)
  batch_dev   the same with the payloads already on the device

The script checks that loop and batch produce the same bytes.  A repetition is `inner` passes over the N frames (at least 64 frames) under a
host clock that ends in a device synchronisation; the forms alternate after a warm-up of each.  Prints per-frame median, minimum, maximum.

--loop-only times the loops alone: they use nothing this change added, so with YK_TREE=<a checkout of the parent commit, built> the same
script times the parent's path on the same machine in the same visit.  --profile runs each batch form once, untimed (for rocprofv3)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("YK_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

args = [a for a in sys.argv[1:] if not a.startswith("--")]
loop_only, profile = "--loop-only" in sys.argv, "--profile" in sys.argv
N, size = int(args[0]), int(args[1])
reps = int(args[2]) if len(args) > 2 else 7
w = h = size
inner = max(1, -(-64 // N))

# ---- the frames: [N, 4, h, w] int32 on the device -------------------------------------------------------------------------------------------------
bx, by, bw, bh = (w // 8) & ~15, h // 8, int(w * 0.7) & ~15, int(h * 0.7)
frames = torch.zeros((N, 4, h, w), dtype=torch.int32, device="cuda")
gen = torch.Generator(device="cuda").manual_seed(5)
for f in range(N):
    frames[f, :3] = synth_planes_torch(w, h, n_planes=3, seed=9000 + (f % 8), device="cuda")
    frames[f, 3, by:by + bh, bx:bx + bw] = torch.randint(1, 255, (bh, bw), generator=gen, device="cuda", dtype=torch.int32)
torch.cuda.synchronize()

one = HipTileEncoder(0)
loop_out = [None] * N


def enc_loop():
    for f in range(N):
        one.set_image(frames[f])
        one.mip_prefilter()
        loop_out[f] = one.alpha_values(True)


def enc_loop_lean():
    for f in range(N):
        one.set_image(frames[f])
        one.alpha_reject()
        one.alpha_finish(None)
        loop_out[f] = one.alpha_values(True)


forms = [("encode loop", enc_loop), ("encode loop_lean", enc_loop_lean)]
batch_out, dev_out = [None], [None]
if not loop_only:
    benc = HipTileEncoder(0)
    benc.set_batch(frames)
    benc.encode_batch()
    benc.synchronize()

    def enc_batch():
        batch_out[0] = benc.alpha_values_batch()

    def enc_batch_dev():
        dev_out[0] = benc.alpha_payloads_device()

    forms += [("encode batch", enc_batch), ("encode batch_dev", enc_batch_dev)]

# ---- decode: the payloads of the encode loop (frame 0's stands for all when the loop has not run yet) ------------------------------------------------
enc_loop_lean()
entries = [(e["mode"], e["bbox"], e["payload"]) for e in loop_out]
assert all(e[0] == 6 for e in entries)
dev_pay = [torch.from_numpy(e[2]).cuda() for e in entries]
dev_entries = [(e[0], e[1], t.data_ptr(), e[2].size) for e, t in zip(entries, dev_pay)]
torch.cuda.synchronize()
dec, bdec = HipTileDecoder(0), HipTileDecoder(0)
out_loop = torch.zeros((N, h, w, 4), dtype=torch.uint8, device="cuda")
out_batch = torch.zeros((N, h, w, 4), dtype=torch.uint8, device="cuda")


def dec_loop():
    for f in range(N):
        dec.begin(w, h)
        dec.decompress_alpha(*entries[f], to_host=False)
        dec.image_device(out_loop[f], channels=4, alpha=-1)


forms.append(("decode loop", dec_loop))
if not loop_only:
    def dec_batch():
        bdec.begin_batch(w, h, N)
        bdec.decompress_alpha_batch(entries, sync=False)
        bdec.image_batch_device(out_batch, channels=4, alpha_from_planes=True)

    def dec_batch_dev():
        bdec.begin_batch(w, h, N)
        bdec.decompress_alpha_batch(dev_entries, sync=False)
        bdec.image_batch_device(out_batch, channels=4, alpha_from_planes=True)

    forms += [("decode batch", dec_batch), ("decode batch_dev", dec_batch_dev)]

handles = [one, dec, bdec] + ([] if loop_only else [benc])


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
    for name, fn in forms:
        if "batch" in name:
            fn()
    fence()
    sys.exit(0)
for _, fn in forms:                                                              # warm-up: code objects, buffers of every handle
    for _ in range(2):
        timed(fn)
ms = {name: [] for name, _ in forms}
for _ in range(reps):
    for name, fn in forms:
        ms[name].append(timed(fn))
if not loop_only:
    enc_loop(); enc_batch(); enc_batch_dev(); benc.synchronize()
    for f in range(N):
        a, b, d = loop_out[f], batch_out[0][f], dev_out[0][f]
        assert a["mode"] == b["mode"] == d[0] and a["bbox"] == b["bbox"] == d[1] and np.array_equal(a["payload"], b["payload"]), f"encode: frame {f} differs"
        got = torch.empty(d[3], dtype=torch.uint8, device="cuda")
        lib_copy = benc._L.yk_device_copy(benc._h, got.data_ptr(), d[2], d[3])
        benc.synchronize()
        assert lib_copy == 0 and np.array_equal(got.cpu().numpy(), a["payload"]), f"encode: frame {f}'s device payload differs"
    dec_loop(); fence(); dec_batch(); fence()
    assert torch.equal(out_loop, out_batch), "decode: batch and loop wrote different pixels"
    out_batch.zero_(); dec_batch_dev(); fence()
    assert torch.equal(out_loop, out_batch), "decode: batch (device payloads) and loop wrote different pixels"
tree = "YK_TREE build" if os.environ.get("YK_TREE") else "this build"
for name, _ in forms:
    v = ms[name]
    print(f"{N} x {w}x{h} RGBA, {tree}, {name:17s}: median {statistics.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; "
          f"{reps} repetitions of {inner * N} frames)", flush=True)
if not loop_only:
    for side in ("encode", "decode"):
        print(f"{N} x {w}x{h} RGBA: {side} batch / loop = {statistics.median(ms[side + ' batch']) / statistics.median(ms[side + ' loop']):.3f}", flush=True)
for x in handles:
    x.close()
