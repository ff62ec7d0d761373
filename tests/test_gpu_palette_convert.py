"""EncoderContext::SetDevicePalette in the C++ mirror (yaik_amd/host): host_driver's `palette` mode converts one image through ConvertHotPath and
through ConvertHotPathBegin / Finish, each with the colour payloads from the host coder (palette.cpp) and from the GPU (yk_palette_compress).
The ZStd library and its inputs are the same, so the four .yaik files must be identical byte for byte."""
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


def test_files_are_identical_with_the_device_palette_off_and_on():
    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-C", os.path.dirname(DRIVER)], check=True)
    planes = synth_planes(256, n_planes=4)
    n, h, w = planes.shape
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.blobs")
        with open(fin, "wb") as f:
            f.write(struct.pack("<3i", w, h, n)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())
        subprocess.run([DRIVER, fin, fout, "palette"], check=True)
        got = parse_blobs(fout)
    host = bytes(got["yaik_host"])
    assert host[:4] == b"YAIK" and len(host) > 1000
    for name in ("yaik_device", "yaik_host_parallel", "yaik_device_parallel"):
        other = bytes(got[name])
        assert len(other) == len(host), (name, len(other), len(host))
        assert other == host, (name, "first difference at byte", next(i for i, (a, b) in enumerate(zip(other, host)) if a != b))
    assert np.frombuffer(got["palette_intervals"], np.int32).tolist() == [2]      # the two device runs went through yk_palette_compress
