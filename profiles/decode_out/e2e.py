"""Per-frame end-to-end decode time from device-resident streams (the encoder's streams where they lie in HBM), run from the repository root as
    python profiles/decode_out/e2e.py <size> [frames]      size = 8192 | 1080 (1920x1080)
Host clock around N frames that end in a device synchronisation; a frame is yk_decode_begin + every gradient chunk + the 1-D chunk, then
  (a) image_into: RGB rows into a host numpy array (de-tile into scratch, 2-D copy over PCIe, host synchronisation per frame);
  (b) image_device: RGB rows into a torch uint8 tensor on the device (no copy, no host synchronisation).
Prints both per-frame times and their difference."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import numpy as np
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

size = sys.argv[1]
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
w, h = (8192, 8192) if size == "8192" else (1920, 1080)
enc = HipTileEncoder(0)
planes = synth_planes_torch(w, h, n_planes=3, seed=12345, device="cuda")
enc.set_image_u8(planes.permute(1, 2, 0).to(torch.uint8).contiguous())
enc.encode(3, False, False)
dec = HipTileDecoder(0)
calls = dec.encoder_streams(enc)
host = np.empty((h, w * 3), np.uint8)
dev = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")


def frame(into_host: bool):
    dec.begin(w, h)
    dec.decode_streams(calls, sync=False)
    if into_host:
        dec.image_into(host)
    else:
        dec.image_device(dev)


def timed(into_host: bool) -> float:
    for _ in range(3):
        frame(into_host)
    torch.cuda.synchronize(); dec.synchronize()
    t = time.perf_counter()
    for _ in range(N):
        frame(into_host)
    torch.cuda.synchronize(); dec.synchronize()
    return (time.perf_counter() - t) / N * 1e3


a, b = timed(True), timed(False)
a2, b2 = timed(True), timed(False)
assert np.array_equal(dev.cpu().numpy().reshape(h, w * 3), host)
print(f"{w}x{h} RGB, {N} frames per run, two runs: (a) image_into host rows {a:.3f} / {a2:.3f} ms per frame; "
      f"(b) image_device {b:.3f} / {b2:.3f} ms per frame; difference {a - b:.3f} / {a2 - b2:.3f} ms "
      f"(image {w * h * 3 / 1e6:.1f} MB)", flush=True)
dec.close(); enc.close()
