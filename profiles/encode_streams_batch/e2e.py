"""decode_batch_from_encoder end to end (the encoder's streams + the batch decode + image_batch_device) per frame, on this build or, with
YK_TREE=<a checkout of the parent commit, built>, on the parent's (measure.sh sets YK_TREE from its own YK_PARENT_TREE for that step): the
default path must not have become slower.  Run from the repository root as
    python profiles/encode_streams_batch/e2e.py <frames> <size> [reps]
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

N, size = int(sys.argv[1]), int(sys.argv[2])
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
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


def timed() -> float:
    torch.cuda.synchronize(); enc.synchronize(); dec.synchronize()
    t = time.perf_counter()
    dec.begin_batch(w, h, N)
    dec.decode_batch_from_encoder(enc, sync=False)
    dec.image_batch_device(out)
    torch.cuda.synchronize(); enc.synchronize(); dec.synchronize()
    return (time.perf_counter() - t) / N * 1e3


for _ in range(2):
    timed()
v = [timed() for _ in range(reps)]
tree = "parent build" if os.environ.get("YK_TREE") else "this build"
print(f"{N} x {w}x{h} RGB, {tree}, decode_batch_from_encoder + image_batch_device: median {statistics.median(v):.4f} ms per frame "
      f"(min {min(v):.4f}, max {max(v):.4f}; {reps} repetitions), checksum {int(out.sum(dtype=torch.int64))}", flush=True)
dec.close(); enc.close()
