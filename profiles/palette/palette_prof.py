"""PaletteCompressor on the GPU against the host coder, on the corner streams of YAIK-synth v1 frames.  Run from the repository root as
    python profiles/palette/palette_prof.py <frames> <size> [reps] [--profile] [--host-frames K]     e.g. 1 8192 | 64 2048

The frames are encoded once (set_batch_u8 + encode_batch) and their corner streams built (streams_batch(corners=True)); then
  (a) colours and distinct voted deltas per pass (frame 0; the votes restated in numpy), payload bytes per pass;
  (b) device  palette_compress_batch(): eight launches + two clears over all 7 x frames streams and one read-back, under a host clock that ends
              with the call (it returns after its read-back); `reps` repetitions after a warm-up, median (min - max); the stage timer
              (YK_STAGE_PALETTE: the launches alone) next to it
      host    yaik_amd/host/palette.cpp (entropy_tool palette: PaletteCompressor alone is timed) on the same streams, one core, from a reset
              book per frame -- what the entropy stage of the parent commit does.  For a batch only the first K frames (default 4) go through
              the host coder, and the figure is scaled to the batch.
      The payloads of the frames that went through both are checked equal.
  --profile runs the device call once, untimed, for a separate rocprofv3 --kernel-trace --stats run."""
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

YK_STAGE_PALETTE = 9
argv = sys.argv[1:]
host_frames = 4
if "--host-frames" in argv:
    i = argv.index("--host-frames")
    host_frames = int(argv[i + 1])
    del argv[i:i + 2]
args = [a for a in argv if not a.startswith("--")]
profile = "--profile" in argv
N, size = int(args[0]), int(args[1])
reps = int(args[2]) if len(args) > 2 else 7
w = h = size
TOOL = os.path.join(ROOT, "yaik_amd", "host", "entropy_tool")

frames = torch.empty((N, h, w, 4), dtype=torch.uint8, device="cuda")
for f in range(N):
    frames[f] = synth_planes_torch(w, h, n_planes=4, seed=12345 + (f % 8), device="cuda").permute(1, 2, 0).to(torch.uint8)
torch.cuda.synchronize()
enc = HipTileEncoder(0)
enc.set_batch_u8(frames)
enc.encode_batch(3, False)
rows = enc.streams_batch(corners=True, range1d=False)
tag = f"{N} x {w}x{h} RGBA"

if profile:
    enc.palette_compress_batch()
    enc.synchronize()
    print(tag, "profiled one palette_compress_batch()")
    sys.exit(0)


def distinct_votes(stream):
    """distinct deltas to the nearest of the 64 colours in front (first minimum), (0,0,0) included once as row 0"""
    c = stream.reshape(-1, 3).astype(np.int32)
    n = len(c)
    if n < 2:
        return 1
    best = np.full(n, 1 << 30, np.int64)
    key = np.zeros(n, np.int64)
    for k in range(min(64, n - 1), 0, -1):                  # ascending prev = descending distance; strict < keeps the first minimum
        d = c[k:] - c[:-k]
        dist = (d.astype(np.int64) ** 2).sum(axis=1)
        better = dist < best[k:]
        best[k:][better] = dist[better]
        key[k:][better] = ((d[:, 0] + 256) | ((d[:, 1] + 256) << 10) | ((d[:, 2] + 256) << 20))[better]
    zero = 256 | (256 << 10) | (256 << 20)
    return len(np.unique(np.concatenate([key[1:], [zero]])))


# ---- (b) device ----
enc.palette_compress_batch()                                 # warm-up: buffers grow here
enc.stage_ms(YK_STAGE_PALETTE)
wall = []
for _ in range(reps):
    t0 = time.perf_counter()
    enc.palette_compress_batch()
    wall.append((time.perf_counter() - t0) * 1e3)
ms, n_int = enc.stage_ms(YK_STAGE_PALETTE)
assert n_int == reps
pay = [[enc.palette_payload(f * 7 + p) for p in range(7)] for f in range(min(N, host_frames))]
raw = [rows[f].download()["rgb"] for f in range(min(N, host_frames))]

# ---- (a) ----
print(f"{tag}: colours / distinct voted deltas / payload bytes per pass (frame 0)")
for p in range(7):
    print(f"  pass {p}: {raw[0][p].size // 3:9d} colours  {distinct_votes(raw[0][p]):8d} deltas  {pay[0][p].size:9d} bytes")
total_colours = sum(sum(rows[f].rgb_bytes) for f in range(N)) // 3
print(f"  all frames: {total_colours} colours, {sum(sum(rows[f].rgb_bytes) for f in range(N))} stream bytes")

# ---- (b) host ----
host_s, host_colours = 0.0, 0
with tempfile.TemporaryDirectory() as d:
    for f in range(len(raw)):
        paths = []
        for p in range(7):
            paths.append(os.path.join(d, f"in{p}"))
            raw[f][p].tofile(paths[-1])
        out = subprocess.run([TOOL, "palette", os.path.join(d, "out"), *paths], check=True, capture_output=True, text=True).stdout
        m = re.search(r"(\d+) colours in ([0-9.]+) s", out)
        host_colours += int(m.group(1)); host_s += float(m.group(2))
        for p in range(7):
            want = np.fromfile(os.path.join(d, f"out{p}"), dtype=np.uint8)
            assert np.array_equal(want, pay[f][p]), ("payload differs", f, p)
scaled = host_s * total_colours / max(host_colours, 1)
print(f"{tag}: device palette_compress_batch() {statistics.median(wall):.3f} ms ({min(wall):.3f} - {max(wall):.3f}), launches alone {ms / reps:.3f} ms per call; "
      f"host palette.cpp on one core {host_s * 1e3:.1f} ms for {len(raw)} frame(s) = {host_colours} colours"
      + (f", scaled to the batch {scaled * 1e3:.1f} ms" if len(raw) < N else "") + f"; ratio {scaled * 1e3 / statistics.median(wall):.0f}x; payloads equal")
