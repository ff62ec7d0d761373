"""Workload behind kernel_stats_6bit_8192.csv, run from the repository root as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o alpha6 -- python profiles/alpha/alpha6_prof.py
yk_alpha_values(force8Bit = 0) on an 8192 x 8192 RGBA image with the analog box of alpha_prof.py: once with every tile of the box kept,
once with 30 % of its 16x16 tiles rejected; five calls of each."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import numpy as np
from yaik_amd.encoder import HipTileEncoder
w = h = 8192
rng = np.random.default_rng(0)
e = HipTileEncoder(0)
for holes in (False, True):
    a = np.zeros((h, w), np.int32)
    a[100:8100, 64:8128] = rng.integers(1, 256, (8000, 8064))
    if holes:
        a[np.kron(rng.random((h // 16, w // 16)) < 0.3, np.ones((16, 16), bool))] = 0
    e.set_image(np.stack([a, a, a, a]))
    e.mip_prefilter()
    for _ in range(5):
        r = e.alpha_values(False)
    print("holes" if holes else "full", r["mode"], r["bbox"], len(r["payload"]))
e.close()
print("encode 6-bit prof done")
