"""PaletteDecompressor on the GPU against the host coder, on the 'GTIL' payloads of YAIK-synth v1 frames.  Run from the repository root as
    python profiles/palette_decode/palette_dec_prof.py <frames> <size> [reps] [--profile] [--host-frames K]     e.g. 1 8192 | 64 2048

The frames are encoded once and their payloads built on the device (streams_batch(corners=True) + palette_compress_batch); then
  device  palette_decompress_streams() over all 7 x frames payloads where the encoder left them + palette_status(), under a host clock;
          `reps` repetitions after a warm-up, median (min - max); the stage timer (YK_STAGE_PALETTE_DEC: the six launches alone) next to it
  host    yaik_amd/host/palette.cpp (entropy_tool unpalette: PaletteDecompressor alone is timed) on the same payloads, one core.  For a batch
          only the first K frames (default 4) go through the host coder, and the figure is scaled to the batch.
  The outputs of the frames that went through both are checked equal.
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

from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

YK_STAGE_PALETTE_DEC = 10
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
enc, dec = HipTileEncoder(0), HipTileDecoder(0)
enc.set_batch_u8(frames)
enc.encode_batch(3, False)
rows = enc.streams_batch(corners=True, range1d=False)
n_pay = enc.palette_compress_batch()
pays = [enc.palette_payload_device(i) for i in range(n_pay)]
outs = [int(rows[i // 7].rgb_bytes[i % 7]) for i in range(n_pay)]
tag = f"{N} x {w}x{h} RGBA"

if profile:
    dec.palette_decompress_streams(pays, outs, 250)
    assert not dec.palette_status().any()
    print(tag, "profiled one palette_decompress_streams()")
    sys.exit(0)

dec.palette_decompress_streams(pays, outs, 250)                  # warm-up: buffers grow here
assert not dec.palette_status().any()
dec.stage_ms(YK_STAGE_PALETTE_DEC)
wall, stage = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    dec.palette_decompress_streams(pays, outs, 250)
    st = dec.palette_status()
    wall.append((time.perf_counter() - t0) * 1e3)
    assert not st.any()
    ms, n_int = dec.stage_ms(YK_STAGE_PALETTE_DEC)                 # behind the clock: one interval per call
    assert n_int == 1
    stage.append(ms)
K = min(N, host_frames)
got = [dec.palette_decoded(i) for i in range(7 * K)]
host_pay = [enc.palette_payload(i) for i in range(7 * K)]
print(f"{tag}: {n_pay} payloads, {sum(p.numel() for p in pays)} payload bytes -> {sum(outs) // 3} colours ({sum(outs)} stream bytes)")

host = []                                                          # seconds for the K frames, one figure per repetition (a fresh process each)
host_colours = 0
with tempfile.TemporaryDirectory() as d:
    for r in range(reps + 1):                                      # the first run is the warm-up
        total, host_colours = 0.0, 0
        for f in range(K):
            cmd = [TOOL, "unpalette", os.path.join(d, "out"), "250"]
            for p in range(7):
                path = os.path.join(d, f"in{p}")
                host_pay[f * 7 + p].tofile(path)
                cmd += [path, str(outs[f * 7 + p])]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
            m = re.search(r"(\d+) colours in ([0-9.]+) s", out)
            host_colours += int(m.group(1)); total += float(m.group(2))
            for p in range(7):
                want = np.fromfile(os.path.join(d, f"out{p}"), dtype=np.uint8)
                assert np.array_equal(want, got[f * 7 + p]), ("output differs", f, p)
        if r:
            host.append(total * 1e3)
scale = (sum(outs) // 3) / max(host_colours, 1)
med = lambda v: f"{statistics.median(v):.3f} ms ({min(v):.3f} - {max(v):.3f})"
print(f"{tag}: device palette_decompress_streams() + palette_status() {med(wall)}, YK_STAGE_PALETTE_DEC alone {med(stage)}; "
      f"host palette.cpp on one core {med(host)} for {K} frame(s) = {host_colours} colours"
      + (f", scaled to the batch {med([h * scale for h in host])}" if K < N else "")
      + f"; ratio of the medians {statistics.median(host) * scale / statistics.median(wall):.1f}x; outputs equal; {reps} repetitions each after a warm-up", flush=True)
dec.close(); enc.close()
