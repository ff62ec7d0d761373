"""The CPU oracle as the yardstick of the ragged-size decode: at sides of 8 (mod 16) its encoder and decoder must agree with each other.
Oracle encode then oracle decode consumes the '1DTL' streams exactly, marks no 4x4 cell outside the image, leaves every in-image cell to
either a gradient tile or the 1-D pass, and reproduces the source."""
import numpy as np
import pytest

from oracle.pyoracle import OracleDecoder, detile
from tests.ragged import SHAPES, cell_marks, oracle_streams, psnr, source, stream_lengths_1d


@pytest.mark.parametrize("w,h,kind", SHAPES)
def test_oracle_round_trip_at_ragged_sizes(oracle_built, w, h, kind):
    planes = source(w, h, kind)
    passes, typ, pix = oracle_streams(planes)
    od = OracleDecoder(w, h)
    for sx, sy, cnt, bm, rgb in passes:
        if cnt:
            assert od.gradient(sx, sy, bm, rgb) == rgb.size             # every corner of the stream is pulled, none past its end
    t4 = od.tile4x4()
    marks = cell_marks(t4, w, h)
    assert not marks[:, w // 4:].any(), "a gradient tile marked cells outside the image"
    # the 1-D streams hold exactly the in-image cells no gradient tile marked
    assert stream_lengths_1d(t4, w, h) == (typ.size, pix.size)
    od.split_masks()
    assert od.decode_1d(typ, pix) == (typ.size, pix.size)
    rec = np.stack([detile(od.planes()[c], w, h) for c in range(3)])
    assert psnr(rec, planes[:3]) > 30.0


def test_stream_lengths_helper_matches_the_oracle_at_multiples_of_16(oracle_built):
    """the helper above, checked where the oracle is pinned against the reference"""
    w, h = 128, 96
    planes = source(w, h, "mixed")
    passes, typ, pix = oracle_streams(planes)
    od = OracleDecoder(w, h)
    for sx, sy, cnt, bm, rgb in passes:
        if cnt:
            od.gradient(sx, sy, bm, rgb)
    assert stream_lengths_1d(od.tile4x4(), w, h) == (typ.size, pix.size)
