"""encode_files_device (YAIK_EncodeImagesFromDevice) of N frames against a loop of N batch-of-one calls on the same encoder.
    python profiles/encode_files/encode_vs_loop.py <frames> <side> <level> <repetitions> [--profile]
The frames are YAIK-synth v1 RGB with an 8-bit alpha box ('ALPM' mode 6), up to 8 distinct ones repeated to fill the batch, uploaded before any
clock starts.  Both forms are timed with a host clock that ends when the last stream is framed (each call returns after that), alternating, after a
warm-up of each.  Prints median and min - max per frame, the split of the batch form's last run from the library's stage clocks
(YAIK_LastEncodeStageMs: device calls, gather + download, entropy + framing), and checks that both forms gave the same streams."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from yaik_amd import files as F  # noqa: E402
from yaik_amd.synth import synth_planes  # noqa: E402


def make_frames(side: int, distinct: int) -> np.ndarray:
    y, x = np.mgrid[0:side, 0:side]
    out = np.empty((distinct, side, side, 4), np.uint8)
    for k in range(distinct):
        out[k, ..., :3] = synth_planes(side, n_planes=3, seed=12345 + k).transpose(1, 2, 0)
        a = np.zeros((side, side), np.uint8)
        x0, y0, x1, y1 = side // 8 + 3, side // 16 + 1, side - side // 16 - 5, side - side // 8 - 7
        a[y0:y1, x0:x1] = ((x * 3 + y * 5 + 17 * k) % 251 + 4)[y0:y1, x0:x1]
        out[k, ..., 3] = a
    return out


def main():
    import torch
    n, side, level, reps = (int(v) for v in sys.argv[1:5])
    profile = "--profile" in sys.argv
    distinct = make_frames(side, min(n, 8))
    frames = torch.from_numpy(distinct).cuda()[torch.arange(n) % distinct.shape[0]].contiguous()
    torch.cuda.synchronize()

    def batch():
        return F.encode_files_device(frames, emit_alpha=True, level=level, threads=16)

    def loop():
        return [F.encode_file_device(frames[f], emit_alpha=True, level=level, threads=16) for f in range(n)]

    a = batch()
    same = profile or a == loop()
    size = sum(map(len, a)) // n
    del a
    tb, tl = [], []
    for _ in range(reps):
        t = time.perf_counter(); batch(); tb.append((time.perf_counter() - t) * 1e3 / n)
        info = F.last_encode_info()
        if not profile:
            t = time.perf_counter(); loop(); tl.append((time.perf_counter() - t) * 1e3 / n)

    def fmt(v):
        return f"{statistics.median(v):.4f} ({min(v):.4f} - {max(v):.4f})" if v else "-"
    print(f"{n} x {side}^2 RGBA level {level}, ms per frame, median (min - max) of {reps}: batch {fmt(tb)}  loop {fmt(tl)}  same streams: {same}  "
          f"last batch run, ms per frame: device calls {info['device_ms'] / n:.4f} gather + download {info['gather_ms'] / n:.4f} "
          f"entropy + framing {info['entropy_ms'] / n:.4f} total {info['total_ms'] / n:.4f}  file bytes per frame: {size}")
    if level == 3 and n == 256 and side == 512 and tl:
        print(f"condition (level 3, 256 x 512^2): batch median {statistics.median(tb):.4f} < loop minimum {min(tl):.4f}: {statistics.median(tb) < min(tl)}")


if __name__ == "__main__":
    main()
