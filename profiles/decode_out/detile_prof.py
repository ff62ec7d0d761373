"""Workload behind profiles/decode_out/kernel_stats_<case>.csv, run from the repository root as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o detile -- python profiles/decode_out/detile_prof.py <case>
case = rgb8192 (HWC RGB) | rgba8192 (HWC RGBA, alpha from the decoded plane) | rgbaconst8192 (HWC RGBA, constant alpha) | chw_rgb8192 (CHW RGB)
| rgba8192_off1 (HWC RGBA from the plane at byte offset 1) | rgba1080 (1920x1080 HWC RGBA from the plane): yk_measure_roof (the measured copy
rate, same process), then ten yk_decode_output_device calls into a torch uint8 tensor, i.e. the de-tile kernel alone.  Prints its event-timed
average (YK_STAGE_DEC_DETILE) and the achieved rate: 3 B/pixel in (+ 1 for an alpha plane) + C out, over kernel time."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import numpy as np
import torch

from yaik_amd._lib import lib
from yaik_amd.decoder import HipTileDecoder

CASES = {"rgb8192": (8192, 8192, 3, None, False, 0), "rgba8192": (8192, 8192, 4, None, False, 0), "rgbaconst8192": (8192, 8192, 4, 255, False, 0),
         "chw_rgb8192": (8192, 8192, 3, None, True, 0), "rgba8192_off1": (8192, 8192, 4, None, False, 1), "rgba1080": (1920, 1080, 4, None, False, 0)}
case = sys.argv[1]
w, h, ch, alpha, planar, off = CASES[case]
d = HipTileDecoder(0)
copy, read = C.c_double(), C.c_double()
assert lib().yk_measure_roof(d._h, 1 << 30, 10, C.byref(copy), C.byref(read)) == 0
d.begin(w, h)                                                   # the planes' content does not matter to a streaming kernel
plane_alpha = ch == 4 and alpha is None
if plane_alpha:
    d.decompress_alpha(6, (0, 0, w, h), np.random.default_rng(1).integers(0, 256, w * h, dtype=np.uint8), to_host=False)
n = off + w * h * ch
buf = torch.empty((n,), dtype=torch.uint8, device="cuda")
out = torch.as_strided(buf, (ch, h, w) if planar else (h, w, ch), (w * h, w, 1) if planar else (w * ch, ch, 1), off)
for _ in range(3):                                              # warm-up: allocations, code objects, the first settle of the planes
    d.image_device(out, channels=ch, alpha=alpha, planar=planar)
torch.cuda.synchronize()
d.stage_ms(5)
for _ in range(10):
    d.image_device(out, channels=ch, alpha=alpha, planar=planar)
torch.cuda.synchronize()
ms, k = d.stage_ms(5)
avg = ms / k
nbytes = (3 + (1 if plane_alpha else 0) + ch) * w * h
print(f"{case}: detile kernel {avg * 1e3:.1f} us (event-timed, {k} calls), {nbytes / 1e6:.1f} MB -> {nbytes / avg / 1e6:.0f} GB/s; "
      f"yk_measure_roof copy {copy.value:.0f} GB/s, read {read.value:.0f} GB/s; "
      f"fraction of copy {nbytes / avg / 1e6 / copy.value:.2f}, of 8 TB/s {nbytes / avg / 1e6 / 8000:.2f}", flush=True)
d.close()
