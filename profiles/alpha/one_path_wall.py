"""Wall time behind one_path_ab.txt, run from the repository root as  python profiles/alpha/one_path_wall.py  (YK_LIB=<library of another
build> selects that build).  HipTileEncoder.alpha_values(True) at 8192 x 8192 on the analog and the binary box of alpha_prof.py: median of 20
calls after 3 warm-up calls, host clock around the call, which synchronises itself.  One line per kind, with a digest of the result."""
import hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import numpy as np
from yaik_amd.encoder import HipTileEncoder
w = h = 8192
rng = np.random.default_rng(0)
e = HipTileEncoder(0)
for kind in ("analog", "binary"):
    a = np.zeros((h, w), np.int32)
    a[100:8100, 64:8128] = rng.integers(0, 256, (8000, 8064)) if kind == "analog" else 255 * rng.integers(0, 2, (8000, 8064))
    e.set_image(np.stack([a, a, a, a]))
    e.mip_prefilter()
    for _ in range(3):
        r = e.alpha_values(True)
    t = []
    for _ in range(20):
        t0 = time.perf_counter()
        r = e.alpha_values(True)
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    dig = hashlib.sha1(r["payload"].tobytes()).hexdigest()[:12]
    print(f"wall {kind} median_ms {(t[9] + t[10]) / 2:.3f} min_ms {t[0]:.3f} max_ms {t[-1]:.3f} mode {r['mode']} bbox {r['bbox']} sha1 {dig}", flush=True)
e.close()
