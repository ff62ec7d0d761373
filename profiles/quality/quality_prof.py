"""Round-trip quality of N equally shaped RGBA frames (YAIK-synth v1), measured where the frames lie: HipTileDecoder.compare_batch_device against
the host route.  Run from the repository root as
    python profiles/quality/quality_prof.py <frames> <size> [reps] [--profile]          e.g. 1 8192 | 64 2048 | 256 512

The frames are encoded (set_batch_u8 + encode_batch) and decoded (decode_batch_from_encoder(alpha=True)) once; then
  (a) the round trip's PSNR and max error per channel against the source, over all frames (one compare call);
  (b) device   compare_batch_device(source): two launches and one read-back of 128 bytes per frame
      host     image_batch_device(channels=4, alpha_from_planes=True).cpu() + numpy on the same frames (the source's host copy is made once,
               outside the timed region: the host route is charged for the decoded frames only)
      seven alternating repetitions after a warm-up, each under a host clock that ends in a device synchronisation; median (min - max).
      The two routes must give equal integers.
  (c) the device time of the two compare launches (YK_STAGE_DEC_COMPARE) next to the de-tile launch of the same shape
      (yk_dec_detile_batch_kernel<4, HWC, PLANE>, YK_STAGE_DEC_DETILE), which moves the same plane bytes plus a pixel stream of the same size
      in the other direction.  --profile runs each of the two once, untimed, for a separate rocprofv3 --kernel-trace --stats run."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.quality import psnr_db
from yaik_amd.synth import synth_planes_torch

YK_STAGE_DEC_DETILE, YK_STAGE_DEC_COMPARE = 5, 8
args = [a for a in sys.argv[1:] if not a.startswith("--")]
profile = "--profile" in sys.argv
N, size = int(args[0]), int(args[1])
reps = int(args[2]) if len(args) > 2 else 7
w = h = size

frames = torch.empty((N, h, w, 4), dtype=torch.uint8, device="cuda")
for f in range(N):
    frames[f] = synth_planes_torch(w, h, n_planes=4, seed=12345 + (f % 8), device="cuda").permute(1, 2, 0).to(torch.uint8)
torch.cuda.synchronize()
enc, dec = HipTileEncoder(0), HipTileDecoder(0)
enc.set_batch_u8(frames)
enc.encode_batch(3, False)
dec.begin_batch(w, h, N)
dec.decode_batch_from_encoder(enc, alpha=True)
tag = f"{N} x {w}x{h} RGBA"


def device_route():
    return dec.compare_batch_device(frames, channels=4)


def detile():
    return dec.image_batch_device(out, channels=4, alpha_from_planes=True)


out = torch.empty_like(frames)
if profile:
    device_route()
    detile()
    torch.cuda.synchronize()
    sys.exit(0)

# (a)
res = device_route()
n = N * w * h
sse = [sum(r["sse"][k] for r in res) for k in range(4)]
print(f"{tag}: round trip vs source, PSNR per channel R G B A = " + " ".join(f"{psnr_db(s, n):.2f}" for s in sse) +
      f" dB, RGB {psnr_db(sum(sse[:3]), 3 * n):.2f} dB, all {psnr_db(sum(sse), 4 * n):.2f} dB; max |err| = {[max(r['max_abs'][k] for r in res) for k in range(4)]}; "
      f"worst frame (RGB) {min(psnr_db(sum(r['sse'][:3]), 3 * w * h) for r in res):.2f} dB", flush=True)

# (b)
src_host = frames.cpu().numpy()


def host_route():
    got = detile().cpu().numpy()
    stats = []
    for f in range(N):
        d = got[f].astype(np.int16) - src_host[f]
        a = np.abs(d)
        stats.append(([int((d[:, :, k].astype(np.int32) ** 2).sum(dtype=np.int64)) for k in range(4)], [int(a[:, :, k].sum(dtype=np.int64)) for k in range(4)],
                      [int(np.count_nonzero(d[:, :, k])) for k in range(4)], [int(a[:, :, k].max()) for k in range(4)]))
    return stats


def timed(fn):
    torch.cuda.synchronize(); dec.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(); dec.synchronize()
    return (time.perf_counter() - t) * 1e3, r


forms = [("device", device_route), ("host", host_route)]
for _, fn in forms:
    timed(fn)
ms = {name: [] for name, _ in forms}
last = {}
for _ in range(reps):
    for name, fn in forms:
        t, last[name] = timed(fn)
        ms[name].append(t)
for f in range(N):
    g, hst = last["device"][f], last["host"][f]
    assert (g["sse"], g["sad"], g["n_diff"], g["max_abs"]) == hst, f"frame {f}: the two routes differ: {g} / {hst}"
for name, _ in forms:
    v = ms[name]
    print(f"{tag}: {name:6s} route: median {statistics.median(v):.3f} ms per call (min {min(v):.3f} - max {max(v):.3f}; {reps} repetitions)", flush=True)
print(f"{tag}: device / host = {statistics.median(ms['device']) / statistics.median(ms['host']):.5f}; equal integers on all {N} frames", flush=True)

# (c)
dec.stage_ms(YK_STAGE_DEC_COMPARE); dec.stage_ms(YK_STAGE_DEC_DETILE)
for _ in range(reps):
    device_route()
    detile()
dec.synchronize()
cmp_ms, k1 = dec.stage_ms(YK_STAGE_DEC_COMPARE)
dt_ms, k2 = dec.stage_ms(YK_STAGE_DEC_DETILE)
moved = N * w * h * (4 + 4)                                                    # 3 plane bytes + 1 alpha byte + 4 pixel bytes per pixel
print(f"{tag}: compare launches {cmp_ms / k1:.4f} ms ({moved / (cmp_ms / k1) / 1e6:.0f} GB/s over {moved / 1e6:.1f} MB read), "
      f"de-tile <4, HWC, PLANE> {dt_ms / k2:.4f} ms ({moved / (dt_ms / k2) / 1e6:.0f} GB/s over the same bytes, half of them written); "
      f"event intervals, mean of {k1}", flush=True)
enc.close(); dec.close()
