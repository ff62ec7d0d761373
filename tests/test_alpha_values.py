"""'ALPM' alpha values on the CPU: the numpy restatement (tests/alpha_ref.py) against the fixtures captured from the reference
(tests/golden/alpha_*.npz: input plane, MipPrefilter bounds and mask, AlphaHeader fields, decompressed payload, unpacker output)."""
import glob
import json
import os

import numpy as np
import pytest

from tests import alpha_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "alpha_*.npz")))


def _load(path):
    return dict(np.load(path))


def test_fixture_set_is_complete():
    names = {os.path.basename(p)[6:-4] for p in FIXTURES}
    assert {"analog_8bit", "analog_6bit_mask", "analog_6bit_fullmask", "binary_ragged", "all255", "low_1to3"} <= names
    for p in FIXTURES:
        prov = json.loads(str(_load(p)["provenance"]))
        assert "EncoderContext.cpp:1429-1682" in prov["encoder"] and prov["capture"]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_encode_matches_reference(path):
    z = _load(path)
    e = R.encode(z["alpha"], z["bounds"], z["mipmask"], bool(z["force8bit"]))
    if not z["has_chunk"]:
        assert e is None
        return
    hd = z["header"]                                   # bbox x, y, w, h, streamSize, expectedDecompressionSize, version, parameters
    assert e is not None
    assert e["mode"] == hd[7] and tuple(e["bbox"]) == tuple(int(v) for v in hd[:4])
    assert len(e["payload"]) == hd[5]
    np.testing.assert_array_equal(e["payload"], z["payload"])


@pytest.mark.parametrize("path", [p for p in FIXTURES if "dec_alpha" in np.load(p)], ids=lambda p: os.path.basename(p))
def test_decode_matches_reference(path):
    z = _load(path)
    h, w = z["alpha"].shape
    hd = z["header"]
    mask = z.get("dec_mask")
    d = R.decode(int(hd[7]), hd[:4], z["payload"], w, h, mask, z.get("dec_mask_bbox"))
    np.testing.assert_array_equal(d, z["dec_alpha"])


def test_binary_ragged_box_is_realigned_to_8():
    z = _load(os.path.join(GOLDEN, "alpha_binary_ragged.npz"))
    x, y, bw, bh = (int(v) for v in z["header"][:4])
    assert z["header"][7] == R.IS_1_BIT_FULL and x % 8 == 0 and bw % 8 == 0
    assert z["header"][5] == bw // 8 * bh


def test_mask_mode_round_trip_finding():
    """6-bit mask mode: the decoder reads the swizzled 'MIPM' mask linearly.  With every tile of the mask box kept, that is all ones
    and the plane comes back (6-bit quantised); with rejected tiles inside the box the reference does not round-trip."""
    q = lambda a: (((a.astype(np.int64) >> 2) << 2) | (a.astype(np.int64) >> 6)).astype(np.uint8)
    full = _load(os.path.join(GOLDEN, "alpha_analog_6bit_fullmask.npz"))
    x, y, bw, bh = (int(v) for v in full["header"][:4])
    want = np.zeros_like(full["alpha"])
    want[y:y + bh, x:x + bw] = q(full["alpha"][y:y + bh, x:x + bw])
    np.testing.assert_array_equal(full["dec_alpha"], want)
    part = _load(os.path.join(GOLDEN, "alpha_analog_6bit_mask.npz"))
    x, y, bw, bh = (int(v) for v in part["header"][:4])
    sel = part["mipmask"][y:y + bh, x:x + bw] != 0
    assert not sel.all()
    assert not np.array_equal(part["dec_alpha"][y:y + bh, x:x + bw][sel], q(part["alpha"][y:y + bh, x:x + bw][sel]))


def test_swizzled_mask_restatement_matches_reference():
    z = _load(os.path.join(GOLDEN, "alpha_analog_6bit_mask.npz"))
    pix_mask = z["mipmask"]
    mb = z["dec_mask_bbox"]
    tx, ty, tbw, tbh = mb[0] >> 4, mb[1] >> 4, mb[2] >> 4, mb[3] >> 4
    tiles = (pix_mask[ty * 16:(ty + tbh) * 16:16, tx * 16:(tx + tbw) * 16:16] != 0).astype(np.uint8).ravel()
    np.testing.assert_array_equal(R.swizzled_mask(np.packbits(tiles, bitorder="little"), tbw, tbh), z["dec_mask"])


@pytest.mark.parametrize("seed", range(6))
def test_restatement_round_trip(seed):
    """encode -> decode in the encoder's layout: 8-bit is exact, binary is exact with w/8 bytes per row."""
    rng = np.random.default_rng(seed)
    h, w = 64, 96
    a = np.zeros((h, w), np.uint8)
    y0, x0 = rng.integers(0, 20, 2)
    if seed % 2:
        a[y0:y0 + 30, x0:x0 + 50] = rng.integers(0, 256, (30, 50))
    else:
        a[y0:y0 + 30, x0:x0 + 50] = 255 * rng.integers(0, 2, (30, 50))
        a[y0, x0] = 255
    e = R.encode(a, (0, 0, w, h), np.ones_like(a), True)
    assert e["mode"] == (R.IS_8_BIT_FULL if seed % 2 else R.IS_1_BIT_FULL)
    d = R.decode(e["mode"], e["bbox"], e["payload"], w, h, reference_1bit=False)
    np.testing.assert_array_equal(d, a)
