"""Workload behind kernel_stats_8192.csv, run from the repository root as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o alpha -- python profiles/alpha/alpha_prof.py
yk_decode_alpha at 8192 x 8192 (8-bit and 1-bit boxes = the whole image, 6-bit mask mode with every tile kept), then yk_alpha_values on an
8192 x 8192 RGBA image with an analog and a binary alpha box; five calls of each."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import numpy as np
from tests import alpha_ref as R
from yaik_amd.decoder import HipTileDecoder
w = h = 8192
d = HipTileDecoder(0)
d.begin(w, h)
rng = np.random.default_rng(0)
pay8 = rng.integers(0, 256, w * h, dtype=np.uint8)
mask = R.swizzled_mask(np.full(w * h // 256 // 8, 255, np.uint8), w // 16, h // 16)
for _ in range(5):
    d.decompress_alpha(R.IS_8_BIT_FULL, (0, 0, w, h), pay8)
    d.decompress_alpha(R.IS_6_BIT_USEMIPMAPMASK_INVERSE, (0, 0, w, h), pay8[: w * h * 3 // 4], mask, (0, 0, w, h))
    d.decompress_alpha(R.IS_1_BIT_FULL, (0, 0, w, h), pay8[: w * h // 8])
d.close()
print("prof done")
# encode: yk_alpha_values on an 8192^2 RGBA image (analog box and binary box)
from yaik_amd.encoder import HipTileEncoder
e = HipTileEncoder(0)
for kind in ("analog", "binary"):
    a = np.zeros((h, w), np.int32)
    a[100:8100, 64:8128] = rng.integers(0, 256, (8000, 8064)) if kind == "analog" else 255 * rng.integers(0, 2, (8000, 8064))
    planes = np.stack([a, a, a, a])
    e.set_image(planes)
    e.mip_prefilter()
    for _ in range(5):
        e.alpha_values(True)
e.close()
print("encode prof done")
