"""'ALPM' 6-bit alpha values on the GPU: yk_alpha_values(force8Bit = 0), i.e. EncoderContext::ProcessAlpha(false), against the fixtures
captured from the reference with force8Bit = 0, the numpy restatement (tests/alpha_ref.py) with the oracle's MipPrefilter mask, the device
decoder, and the ConvertHotPath alpha6Bit option through YAIK_DecodeImage."""
import os
import subprocess

import numpy as np
import pytest

from tests import alpha_ref as R
from tests.test_alpha_6bit_mask import shape_alpha, tile_keep, tile_mask
from tests.test_gpu_alpha_values import TAG_ALPM, _chunks, _decode_file, _planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIX_BIT = ["alpha_analog_6bit_mask.npz", "alpha_analog_6bit_fullmask.npz"]


@pytest.fixture(scope="module")
def enc():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dec():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


def tile_bounds(alpha):
    """the MipPrefilter bounds of the GPU alpha stage: the box of the kept 16x16 tiles"""
    ys, xs = np.nonzero(tile_keep(alpha))
    return np.array([xs.min() * 16, ys.min() * 16, xs.max() * 16 + 16, ys.max() * 16 + 16], np.int32)


def _same(got, want):
    if want is None:
        assert got is None
        return
    assert got is not None and got["mode"] == want["mode"] and got["bbox"] == tuple(int(v) for v in want["bbox"])
    np.testing.assert_array_equal(got["payload"], want["payload"])


def _check(enc, alpha, mask=None):
    """GPU 6-bit encode of `alpha` against the restatement on the GPU's bounds; mask = the per-pixel mipmapMask (default: the tile rule)."""
    enc.set_image(_planes(alpha))
    mp = enc.mip_prefilter()
    got = enc.alpha_values(False)
    m = tile_mask(alpha, mp["bounds"]) if mask is None else mask
    want = R.encode(alpha, mp["bounds"], m, False)
    _same(got, want)
    if want is not None and want["mode"] != R.IS_6_BIT_USEMIPMAPMASK_INVERSE:     # force8Bit does not touch these branches
        _same(enc.alpha_values(True), want)
    return mp, got


@pytest.mark.parametrize("name", SIX_BIT)
def test_gpu_encode_6bit_matches_fixture(enc, name):
    z = dict(np.load(os.path.join(GOLDEN, name)))
    # the captured mask inside the captured bounds; outside them (the reference's bounds are clipped on these non-square images, the
    # GPU's are not) the reference's recursion never visits the mask, so the tile rule pinned in tests/test_alpha_6bit_mask.py applies
    a = z["alpha"]
    mask = tile_mask(a, tile_bounds(a))
    x0, y0, x1, y1 = (int(v) for v in z["bounds"])
    mask[y0:y1, x0:x1] = z["mipmask"][y0:y1, x0:x1] != 0
    mp, got = _check(enc, a, mask)
    np.testing.assert_array_equal(mp["bounds"], tile_bounds(a))
    assert got["mode"] == R.IS_6_BIT_USEMIPMAPMASK_INVERSE
    if np.array_equal(mp["bounds"], z["bounds"]):      # the search region is the reference's: header and payload are too
        hd = z["header"]
        assert got["bbox"] == tuple(int(v) for v in hd[:4]) and len(got["payload"]) == hd[5]
        np.testing.assert_array_equal(got["payload"], z["payload"])


def _kinds(rng, h, w):
    """(name, alpha) cases on an h x w plane: rejected tiles inside the box, narrow content, every alpha class"""
    out = []
    a = np.zeros((h, w), np.int32)                     # ring of tiles around an empty core
    y0, x0 = int(rng.integers(0, 3)) * 8, int(rng.integers(0, 3)) * 8
    a[y0:h - 2, x0:w - 3] = rng.integers(0, 256, (h - 2 - y0, w - 3 - x0))
    a[y0 + 20:h - 22, x0 + 21:w - 24] = 0
    out.append(("ring", a))
    a = np.zeros((h, w), np.int32)                     # L shape
    a[3:h, 5:22] = rng.integers(0, 256, (h - 3, 17))
    a[h - 19:h - 1, 5:w - 1] = rng.integers(0, 256, (18, w - 6))
    out.append(("L", a))
    for width in (1, 2, 3):                            # content 1..3 samples wide before the rounding to 4
        a = np.zeros((h, w), np.int32)
        x = int(rng.integers(0, w - width))
        a[4:h - 4, x:x + width] = rng.integers(4, 255, (h - 8, width))
        out.append((f"narrow{width}", a))
    a = np.zeros((h, w), np.int32)                     # scattered tiles
    for _ in range(6):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        a[y:y + int(rng.integers(1, 30)), x:x + int(rng.integers(1, 30))] = rng.integers(0, 256)
    a[int(rng.integers(0, h)), int(rng.integers(0, w))] = 77
    out.append(("scatter", a))
    a = np.full((h, w), 0, np.int32)                   # spans the image with an empty tile inside: no 'MIPM', every pixel selected
    a[:] = rng.integers(0, 256, (h, w))
    a[16:32, 16:32] = 0
    a[0, 0] = a[h - 1, w - 1] = 9
    out.append(("holed", a))
    b = np.zeros((h, w), np.int32)
    b[2:h - 5, 7:w - 9] = 255 * rng.integers(0, 2, (h - 7, w - 16))
    b[2, 7] = 255
    out += [("binary", b), ("all255", np.full((h, w), 255, np.int32)), ("empty", np.zeros((h, w), np.int32))]
    return out


@pytest.mark.parametrize("seed", range(8))
def test_gpu_encode_6bit_fuzz_odd_shapes(enc, seed):
    """shapes that are multiples of 8 but not of 16 (clipped edge tiles); the mask is the tile rule tests/test_alpha_6bit_mask.py pins"""
    rng = np.random.default_rng(6000 + seed)
    h, w = int(rng.integers(4, 14)) * 16 + 8, int(rng.integers(4, 14)) * 16 + 8
    for _, a in _kinds(rng, h, w):
        _check(enc, a)


@pytest.mark.parametrize("seed", range(6))
def test_gpu_encode_6bit_fuzz_oracle_mask(enc, oracle_built, seed):
    """square power-of-two planes, where the oracle's MipPrefilter is defined: the mask is its mipmapMask"""
    rng = np.random.default_rng(6100 + seed)
    n = (64, 128, 256)[seed % 3]
    cases = _kinds(rng, n, n) + [(k, shape_alpha(rng, n, k)) for k in ("ring", "L", "holed")]
    for name, a in cases:
        o = oracle_built.OracleEncoder(_planes(a))
        omp = o.mip_prefilter()
        mp, _ = _check(enc, a, (o.state("mipmapMask") != 0).astype(np.uint8))
        np.testing.assert_array_equal(mp["bounds"], omp["bounds"], err_msg=name)


def _check_large(enc, alpha_u8):
    """full-size planes: the planes are built on the device; the restatement runs on the bounds' crop (x offset a multiple of 16, so the
    rounding to 4 and 8 is the same) and its box is shifted back"""
    import torch
    h, w = alpha_u8.shape
    planes = torch.zeros((4, h, w), dtype=torch.int32, device="cuda")
    planes[3].copy_(torch.from_numpy(alpha_u8).to("cuda").to(torch.int32))
    enc.set_image(planes)
    mp = enc.mip_prefilter()
    got = enc.alpha_values(False)
    del planes
    x0, y0, x1, y1 = (int(v) for v in mp["bounds"])
    x1, y1 = min(x1, w), min(y1, h)
    crop = alpha_u8[y0:y1, x0:x1]
    if tuple(mp["bounds"]) == (0, 0, w, h):
        mask = np.ones_like(crop)
    else:
        keep = tile_keep(alpha_u8)
        mask = np.kron(keep[y0 // 16:(y1 + 15) // 16, x0 // 16:(x1 + 15) // 16], np.ones((16, 16), np.uint8))[:y1 - y0, :x1 - x0]
    want = R.encode(crop, (0, 0, x1 - x0, y1 - y0), mask, False)
    want["bbox"] = (want["bbox"][0] + x0, want["bbox"][1] + y0, want["bbox"][2], want["bbox"][3])
    assert want["mode"] == R.IS_6_BIT_USEMIPMAPMASK_INVERSE
    _same(got, want)


def test_gpu_encode_6bit_8192(enc):
    rng = np.random.default_rng(8192)
    n = 8192
    a = np.zeros((n, n), np.uint8)
    a[1000:7001, 333:8000] = rng.integers(0, 256, (6001, 7667), dtype=np.uint8)
    tiles = rng.random((n // 16, n // 16)) < 0.3      # rejected tiles all over the box
    a[np.kron(tiles, np.ones((16, 16), bool))] = 0
    _check_large(enc, a)


def test_gpu_encode_6bit_16384(enc):
    rng = np.random.default_rng(16384)
    n = 16384
    a = np.zeros((n, n), np.uint8)
    a[3000:5003, 21:16370] = rng.integers(0, 256, (2003, 16349), dtype=np.uint8)   # > 1000 tile columns per band
    a[3100:4900, 3000:9000] = 0
    _check_large(enc, a)


def _decoder_selected(mask, mbox, bbox):
    """samples the decoder's mask modes select: the swizzled mask read linearly from the box origin with stride mbox.w (as R.decode)"""
    bx, by, bw, bh = (int(v) for v in bbox)
    stride = int(mbox[2])
    r, c = np.mgrid[0:bh, 0:bw]
    pos = (bx - int(mbox[0])) + stride * (by - int(mbox[1])) + stride * r.astype(np.int64) + c
    inside = (pos >> 3) < mask.size
    return int((((mask[pos[inside] >> 3] >> (pos[inside] & 7)) & 1) != 0).sum())


@pytest.mark.parametrize("kind", ["ring", "full"])
def test_gpu_6bit_round_trip_through_device_decoder(enc, dec, kind):
    """the payload through yk_decode_alpha with the swizzled 'MIPM' mask equals the restated decoder; with every tile kept it is the source
    6-bit quantised inside the box"""
    rng = np.random.default_rng(44)
    h, w = 128, 160
    a = np.zeros((h, w), np.int32)
    a[20:100, 36:130] = rng.integers(0, 256, (80, 94))
    if kind == "ring":
        a[48:80, 64:112] = 0
    enc.set_image(_planes(a))
    mp = enc.mip_prefilter()
    assert mp["has_chunk"]
    got = enc.alpha_values(False)
    tb = mp["tile_bbox"]
    mask = R.swizzled_mask(mp["bitmap"], int(tb[2]), int(tb[3]))
    mbox = tuple(int(v) * 16 for v in tb)
    dec.begin(w, h)
    pay = got["payload"]
    need = (_decoder_selected(mask, mbox, got["bbox"]) * 6 + 7) // 8
    if kind == "ring":
        # the mask-mode finding: the decoder reads the swizzled mask linearly and selects more samples than the encoder wrote,
        # so it refuses the payload as it is; padded with zero bytes (what the restated decoder reads past the end) it decodes
        assert need > len(pay)
        from yaik_amd._lib import YaikError
        with pytest.raises(YaikError):
            dec.decompress_alpha(got["mode"], got["bbox"], pay, mask, mbox)
    fed = np.concatenate([pay, np.zeros(max(0, need - len(pay)), np.uint8)])
    plane = dec.decompress_alpha(got["mode"], got["bbox"], fed, mask, mbox)
    np.testing.assert_array_equal(plane, R.decode(got["mode"], got["bbox"], pay, w, h, mask, mbox))
    if kind == "full":
        x, y, bw, bh = got["bbox"]
        want = np.zeros((h, w), np.uint8)
        v = a[y:y + bh, x:x + bw]
        want[y:y + bh, x:x + bw] = ((v >> 2) << 2) | (v >> 6)
        np.testing.assert_array_equal(plane, want)


# ---- ConvertHotPath with emitAlpha + alpha6Bit, YAIK_DecodeImage ----------------------------------------------------------------------------
ADRV = os.path.join(ROOT, "yaik_amd", "host", "alpha_driver")


@pytest.fixture(scope="module")
def adrv():
    subprocess.run(["make", "-C", os.path.join(ROOT, "yaik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return ADRV


def _encode(adrv, planes, tmp, emit, *opts):
    import struct
    n, h, w = planes.shape
    fin, fy = os.path.join(tmp, "in6.bin"), os.path.join(tmp, "out6.yaik")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", w, h, n)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())
    subprocess.run([adrv, "enc", fin, fy, "1" if emit else "0", *opts], check=True)
    with open(fy, "rb") as f:
        return f.read()


def _alpm_mode(data):
    p, _, _ = next(c for c in _chunks(data) if c[1] == TAG_ALPM)
    return data[p + 8 + 17] & 7


def _strip_alpm(data):
    p, _, ln = next(c for c in _chunks(data) if c[1] == TAG_ALPM)
    return data[:p] + data[p + 8 + ln:]


def test_convert_alpha6_full_box_is_mask_mode(adrv, tmp_path):
    rng = np.random.default_rng(61)
    h, w = 96, 128
    a = np.zeros((h, w), np.int32)
    a[16:80, 32:112] = rng.integers(0, 256, (64, 80))   # every tile of the 'MIPM' box kept
    a[16, 32] = a[79, 111] = 200
    planes = _planes(a)
    six = _encode(adrv, planes, str(tmp_path), True, "alpha6")
    assert _alpm_mode(six) == R.IS_6_BIT_USEMIPMAPMASK_INVERSE
    assert _encode(adrv, planes, str(tmp_path), True, "parallel", "alpha6") == six
    eight = _encode(adrv, planes, str(tmp_path), True)
    assert _alpm_mode(eight) == R.IS_8_BIT_FULL and _strip_alpm(six) == _strip_alpm(eight)
    d = _decode_file(adrv, six, str(tmp_path))
    assert d["ok"] and d["bpp"] == 4
    x0, x1 = (32 >> 2) << 2, 112
    want = np.zeros((h, w), np.uint8)
    v = a[16:80, x0:x1]
    want[16:80, x0:x1] = ((v >> 2) << 2) | (v >> 6)
    want[a >> 2 == 0] = 0
    np.testing.assert_array_equal(d["image"][..., 3], want)
    np.testing.assert_array_equal(d["plane_a"], want)


def test_convert_alpha6_ring_falls_back_to_8bit(adrv, tmp_path):
    rng = np.random.default_rng(62)
    h, w = 96, 128
    a = np.zeros((h, w), np.int32)
    a[16:80, 32:112] = rng.integers(0, 256, (64, 80))
    a[32:64, 48:96] = 0                                 # rejected tiles inside the box
    planes = _planes(a)
    six = _encode(adrv, planes, str(tmp_path), True, "alpha6")
    assert _alpm_mode(six) == R.IS_8_BIT_FULL
    assert six == _encode(adrv, planes, str(tmp_path), True)
    d = _decode_file(adrv, six, str(tmp_path))
    assert d["ok"]
    np.testing.assert_array_equal(d["image"][..., 3], a.astype(np.uint8))


def test_convert_alpha6_without_mipm_falls_back_to_8bit(adrv, tmp_path):
    a = np.full((64, 64), 128, np.int32)               # kept tiles span the image: no 'MIPM' chunk
    planes = _planes(a)
    six = _encode(adrv, planes, str(tmp_path), True, "alpha6")
    assert _chunks(six)[0][1] == TAG_ALPM and _alpm_mode(six) == R.IS_8_BIT_FULL
    assert six == _encode(adrv, planes, str(tmp_path), True)


def test_convert_alpha6_off_is_unchanged(adrv, tmp_path):
    """alpha6Bit without emitAlpha writes no 'ALPM' chunk and changes nothing; without alpha6Bit the file is the one the driver always wrote"""
    import struct
    rng = np.random.default_rng(63)
    a = np.zeros((96, 128), np.int32)
    a[16:80, 32:112] = rng.integers(0, 256, (64, 80))
    planes = _planes(a)
    off = _encode(adrv, planes, str(tmp_path), False)
    assert _encode(adrv, planes, str(tmp_path), False, "alpha6") == off
    fin, fb, fy = str(tmp_path / "h.bin"), str(tmp_path / "h.blobs"), str(tmp_path / "h.yaik")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", 128, 96, 4)); f.write(planes.tobytes())
    subprocess.run([os.path.join(ROOT, "yaik_amd", "host", "host_driver"), fin, fb, "0", fy], check=True, stdout=subprocess.DEVNULL)
    assert open(fy, "rb").read() == off
    on = _encode(adrv, planes, str(tmp_path), True)
    assert _alpm_mode(on) == R.IS_8_BIT_FULL and _strip_alpm(on) == off
