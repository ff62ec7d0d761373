"""Workload behind profiles/pixels/kernel_stats_<case>.csv, run from the repository root as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o unpack -- python profiles/pixels/unpack_prof.py <case>
case = rgba8192 | rgb8192 | rgba1080, or one of them + "_off1" (the same pixels at byte offset 1: the byte path): yk_measure_roof (the measured
copy rate, same process), then ten yk_load_device_pixels_u8 calls on torch uint8 pixels already in HBM, i.e. the unpack kernel alone.  Prints
its event-timed average (YK_STAGE_UNPACK) and the achieved rate, (channels + 4 * nPlanes) * w * h bytes over kernel time."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import torch

from yaik_amd.encoder import HipTileEncoder

CASES = {"rgba8192": (8192, 8192, 4), "rgb8192": (8192, 8192, 3), "rgba1080": (1920, 1080, 4)}
case = sys.argv[1]
w, h, ch = CASES[case.replace("_off1", "")]
off = 1 if case.endswith("_off1") else 0
e = HipTileEncoder(0)
copy, read = C.c_double(), C.c_double()
assert e._L.yk_measure_roof(e._h, 1 << 30, 10, C.byref(copy), C.byref(read)) == 0
buf = torch.randint(0, 256, (off + h * w * ch,), dtype=torch.uint8, device="cuda")
px = torch.as_strided(buf, (h, w, ch), (w * ch, ch, 1), off)
for _ in range(3):                                              # warm-up: allocations, code objects
    e.set_image_u8(px)
e.synchronize()
e.stage_ms(7)
for _ in range(10):
    e.set_image_u8(px)
ms, n = e.stage_ms(7)
avg = ms / n
nbytes = (ch + 4 * ch) * w * h
print(f"{case}: unpack kernel {avg * 1e3:.1f} us (event-timed, {n} calls), {nbytes / 1e6:.1f} MB -> {nbytes / avg / 1e6:.0f} GB/s; "
      f"yk_measure_roof copy {copy.value:.0f} GB/s, read {read.value:.0f} GB/s; "
      f"fraction of copy {nbytes / avg / 1e6 / copy.value:.2f}, of 8 TB/s {nbytes / avg / 1e6 / 8000:.2f}", flush=True)
e.close()
