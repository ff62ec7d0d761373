"""decode_batch_from_encoder end to end (the encoder's streams + the batch decode + image_batch_device) per frame, with the corner streams taken
as they are (palette=False, the default) or through the 'GTIL' payloads (--palette: palette_compress_batch on the encoder once, before the
clock starts, then palette_decompress_streams on the decoder in every repetition), on this build or, with YK_TREE=<a checkout of the parent commit, built>, on the parent's (default
path only): the default path must not have moved.  Run from the repository root as
    python profiles/palette_decode/e2e.py <frames> <size> [reps] [--palette]
The encoder is encoded once, before the clock starts; a repetition ends in a device synchronisation."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("YK_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

palette = "--palette" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
N, size = int(args[0]), int(args[1])
reps = int(args[2]) if len(args) > 2 else 7
w = h = size
enc, dec = HipTileEncoder(0), HipTileDecoder(0)
frames = torch.empty((N, h, w, 3), dtype=torch.uint8, device="cuda")
for f in range(N):
    frames[f] = synth_planes_torch(w, h, n_planes=3, seed=9000 + f, device="cuda").permute(1, 2, 0).to(torch.uint8)
torch.cuda.synchronize()
enc.set_batch_u8(frames)
enc.encode_batch(3, False)
enc.synchronize()
out = torch.zeros((N, h, w, 3), dtype=torch.uint8, device="cuda")
kw = {"palette": True} if palette else {}
if palette:                                     # the payloads are the caller's to make, once: nothing below encodes again
    enc.streams_batch()
    enc.palette_compress_batch()
    enc.synchronize()


def timed() -> float:
    torch.cuda.synchronize(); enc.synchronize(); dec.synchronize()
    t = time.perf_counter()
    dec.begin_batch(w, h, N)
    dec.decode_batch_from_encoder(enc, sync=False, **kw)
    dec.image_batch_device(out)
    torch.cuda.synchronize(); enc.synchronize(); dec.synchronize()
    return (time.perf_counter() - t) / N * 1e3


for _ in range(2):
    timed()
v = [timed() for _ in range(reps)]
tree = "parent build" if os.environ.get("YK_TREE") else "this build"
print(f"{N} x {w}x{h} RGB, {tree}, palette={palette}, decode_batch_from_encoder + image_batch_device: median {statistics.median(v):.4f} ms per frame "
      f"(min {min(v):.4f}, max {max(v):.4f}; {reps} repetitions), checksum {int(out.sum(dtype=torch.int64))}", flush=True)
dec.close(); enc.close()
