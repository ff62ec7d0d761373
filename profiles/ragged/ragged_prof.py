"""Workload behind kernel_stats_1920x1080.csv and kernel_stats_1920x1088.csv, run from the repository root as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ragged -- python profiles/ragged/ragged_prof.py <height>
One 1920 x <height> RGB frame (tests/ragged.py's "photo" image) encoded once on the GPU, then decoded 20 times from the encoder's
device-resident streams (HipTileDecoder.decode_from_encoder: one yk_decode_gradient_all_device call + yk_decode_1d_device) and written out
as RGB rows.  1080 = 8 (mod 16) is the ragged case, 1088 the next multiple of 16: the same kernels, 0.7 % more pixels."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import numpy as np
from tests.images import edge_image
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
w, h = 1920, int(sys.argv[1]) if len(sys.argv) > 1 else 1080
planes = edge_image(w, h, "photo", 3, seed=w * 7 + h)
e, d = HipTileEncoder(0), HipTileDecoder(0)
e.set_image(planes)
e.encode(3, False, False)
calls = d.encoder_streams(e)
out = np.zeros((h, w * 3), np.uint8)
for _ in range(20):
    d.begin(w, h)
    d.decode_streams(calls)
    d.image_into(out)
print(w, h, "decoded", int(out.sum()) % 1000003)
d.close(); e.close()
print("ragged decode prof done")
