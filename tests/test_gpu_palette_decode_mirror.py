"""YAIK_SetDevicePalette in the C++ mirror (yaik_amd/host/yaik_decode.cpp): host_driver's `decode_palette` mode decodes one .yaik stream with
PaletteDecompressor on the host (palette.cpp) and on the GPU (yk_decode_gradient_palette), and a copy of the stream whose first 'GTIL' payload was
made malformed.  The images must be identical, and the malformed copy must fail with YAIK_INVALID_STREAM both ways."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from oracle.refrun import parse_blobs
from tests.images import synth_planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "yaik_amd", "host", "host_driver")
YAIK_INVALID_STREAM = 6


def test_images_are_identical_and_a_malformed_payload_is_an_invalid_stream_both_ways():
    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-C", os.path.dirname(DRIVER)], check=True)
    planes = synth_planes(256, n_planes=4)
    n, h, w = planes.shape
    with tempfile.TemporaryDirectory() as d:
        fin, fout, fy, fdec = (os.path.join(d, x) for x in ("in.bin", "out.blobs", "a.yaik", "dec.blobs"))
        with open(fin, "wb") as f:
            f.write(struct.pack("<3i", w, h, n)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())
        subprocess.run([DRIVER, fin, fout, "palette"], check=True)
        with open(fy, "wb") as f:
            f.write(bytes(parse_blobs(fout)["yaik_host"]))
        subprocess.run([DRIVER, "decode_palette", fdec, fy], check=True)
        got = parse_blobs(fdec)
    info = {k: np.frombuffer(got["pal_info_" + k], np.int32).tolist() for k in ("off", "on", "bad_off", "bad_on")}
    assert info["off"][:4] == [1, 0, w, h] and info["on"] == info["off"], info
    off, on = np.frombuffer(got["pal_image_off"], np.uint8), np.frombuffer(got["pal_image_on"], np.uint8)
    assert off.size == w * h * info["off"][4] and int(off.max()) > 0
    assert np.array_equal(off, on)
    for k in ("bad_off", "bad_on"):
        assert info[k][:2] == [0, YAIK_INVALID_STREAM], (k, info[k])
