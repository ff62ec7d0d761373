"""decode_files_device (YAIK_DecodeImagesToDevice) against a loop of decode_file_device (YAIK_DecodeImageToDevice) on the same streams.
    python profiles/decode_files/batch_vs_loop.py <frames> <side> <repetitions> [--profile]
The streams are YAIK-synth v1 RGBA frames with 8-bit alpha ('ALPM' mode 6), written once by ConvertHotPath (alpha_driver enc) before any clock
starts: up to 8 distinct files, repeated to fill the batch.  Both forms write device memory and are timed with a host clock that ends in a device
synchronise (each call returns after one), alternating, after a warm-up of each.  Prints median and min - max per frame, the split of the batch
form's last run (host expansion, upload, batch calls) from the library's stage clocks, and checks that both forms wrote the same bytes."""
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from yaik_amd import files as F  # noqa: E402
from yaik_amd.synth import synth_planes  # noqa: E402


def make_files(side: int, distinct: int) -> list:
    adrv = os.path.join(ROOT, "yaik_amd", "host", "alpha_driver")
    out = []
    with tempfile.TemporaryDirectory() as d:
        for k in range(distinct):
            planes = synth_planes(side, n_planes=4, seed=12345 + k)
            fin, fy = os.path.join(d, "in.bin"), os.path.join(d, "out.yaik")
            with open(fin, "wb") as f:
                f.write(struct.pack("<3i", side, side, 4)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())
            subprocess.run([adrv, "enc", fin, fy, "1"], check=True)
            out.append(open(fy, "rb").read())
    return out


def main():
    import torch
    n, side, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    profile = "--profile" in sys.argv
    distinct = make_files(side, min(n, 8))
    streams = [distinct[i % len(distinct)] for i in range(n)]
    out = torch.empty((n, side, side, 4), dtype=torch.uint8, device="cuda")

    def batch():
        F.decode_files_device(streams, out=out, channels=4, threads=16)

    def loop():
        return [F.decode_file_device(s) for s in streams]

    batch(); ref = loop(); torch.cuda.synchronize()
    same = all(bool((out[i][..., :r.shape[2]] == r).all()) and (r.shape[2] == 4 or bool((out[i][..., 3] == 255).all())) for i, r in enumerate(ref))
    del ref
    tb, tl = [], []
    for _ in range(reps):
        t = time.perf_counter(); batch(); tb.append((time.perf_counter() - t) * 1e3 / n)
        info = F.last_batch_info()
        if not profile:
            t = time.perf_counter(); loop(); tl.append((time.perf_counter() - t) * 1e3 / n)

    def fmt(v):
        return f"{statistics.median(v):.4f} ({min(v):.4f} - {max(v):.4f})" if v else "-"
    print(f"{n} x {side}^2 RGBA, ms per frame, median (min - max) of {reps}: batch {fmt(tb)}  loop {fmt(tl)}  same bytes: {same}  "
          f"fallbacks: {info['fallbacks']}  last batch run, ms per frame: expand {info['expand_ms'] / n:.4f} upload {info['upload_ms'] / n:.4f} "
          f"batch calls {info['decode_ms'] / n:.4f}  file bytes per frame: {sum(map(len, streams)) // n}")


if __name__ == "__main__":
    main()
