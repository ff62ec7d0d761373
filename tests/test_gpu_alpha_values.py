"""'ALPM' alpha values on the GPU (yk_decode_alpha): the device unpacker against the reference's unpacker output (fixtures) and the
numpy restatement (tests/alpha_ref.py), its error paths, and the RGBA image built from the plane left in HBM."""
import glob
import os

import numpy as np
import pytest

from tests import alpha_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNKED = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "alpha_*.npz"))) if int(np.load(p)["has_chunk"])]


@pytest.fixture(scope="module")
def dec():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.mark.parametrize("path", CHUNKED, ids=lambda p: os.path.basename(p))
def test_gpu_decode_matches_reference(dec, path):
    z = dict(np.load(path))
    h, w = z["alpha"].shape
    hd = z["header"]
    mode = int(hd[7])
    mask, mbox = z.get("dec_mask"), z.get("dec_mask_bbox")
    dec.begin(w, h)
    got = dec.decompress_alpha(mode, hd[:4], z["payload"], mask, mbox, reference_1bit=True)
    want = z["dec_alpha"] if "dec_alpha" in z else R.decode(mode, hd[:4], z["payload"], w, h, mask, mbox)
    np.testing.assert_array_equal(got, want)
    if mode == R.IS_1_BIT_FULL:                        # the encoder's layout decodes back to the source
        got = dec.decompress_alpha(mode, hd[:4], z["payload"])
        x, y, bw, bh = (int(v) for v in hd[:4])
        exp = np.zeros_like(z["alpha"])
        exp[y:y + bh, x:x + bw] = np.where(z["alpha"][y:y + bh, x:x + bw] & 1, 255, 0)
        np.testing.assert_array_equal(got, exp)


def _case(rng, w, h, mode, cap=1 << 30):
    bw = int(rng.integers(1, min(w, cap) // 8)) * 8
    bh = int(rng.integers(1, min(h, cap)))
    bx = int(rng.integers(0, (w - bw) // 8 + 1)) * 8
    by = int(rng.integers(0, h - bh + 1))
    if mode == R.IS_8_BIT_FULL:
        n = bw * bh
    elif mode == R.IS_1_BIT_FULL:
        n = bw // 8 * bh
    else:
        n = bw // 4 * 3 * bh
    return (bx, by, bw, bh), rng.integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("size", [(8192, 8192), (16384, 16384)])
@pytest.mark.parametrize("mode", [R.IS_1_BIT_FULL, R.IS_6_BIT_FULL, R.IS_6_BIT_FULL_INVERSE, R.IS_8_BIT_FULL])
def test_gpu_decode_large_vs_restatement(dec, size, mode):
    w, h = size
    rng = np.random.default_rng(mode * 7 + w)
    bbox, pay = _case(rng, w, h, mode, cap=6144)     # the whole plane is checked; the box keeps the numpy side in memory
    dec.begin(w, h)
    got = dec.decompress_alpha(mode, bbox, pay)
    np.testing.assert_array_equal(got, R.decode(mode, bbox, pay, w, h, reference_1bit=False))


@pytest.mark.parametrize("seed", range(8))
def test_gpu_decode_fuzz(dec, seed):
    """random shapes, boxes, modes, masks (fixed seeds, one run each); the 1-bit mode in both layouts"""
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(1, 40)) * 16, int(rng.integers(1, 40)) * 16
    dec.begin(w, h)
    for mode in (R.IS_1_BIT_FULL, R.IS_6_BIT_FULL, R.IS_6_BIT_FULL_INVERSE, R.IS_8_BIT_FULL):
        bbox, pay = _case(rng, w, h, mode)
        for quirk in ((False, True) if mode == R.IS_1_BIT_FULL else (False,)):
            if quirk and bbox[2] == 8:
                continue
            got = dec.decompress_alpha(mode, bbox, pay, reference_1bit=quirk)
            np.testing.assert_array_equal(got, R.decode(mode, bbox, pay, w, h, reference_1bit=quirk))
    # mask modes: a random tile mask, its swizzled decoder form, an alpha box inside the mask box
    tbw, tbh = int(rng.integers(1, w // 16 + 1)), int(rng.integers(1, h // 16 + 1))
    tx, ty = int(rng.integers(0, w // 16 - tbw + 1)), int(rng.integers(0, h // 16 - tbh + 1))
    tiles = rng.integers(0, 2, tbw * tbh).astype(np.uint8)
    mask = R.swizzled_mask(np.packbits(tiles, bitorder="little"), tbw, tbh)
    mbox = (tx * 16, ty * 16, tbw * 16, tbh * 16)
    bw = int(rng.integers(1, tbw * 4 + 1)) * 4
    bh = int(rng.integers(1, tbh * 16 + 1))
    bx = tx * 16 + int(rng.integers(0, (tbw * 16 - bw) // 4 + 1)) * 4
    by = ty * 16 + int(rng.integers(0, tbh * 16 - bh + 1))
    pay = rng.integers(0, 256, bw * bh, dtype=np.uint8)
    for mode in (R.IS_6_BIT_USEMIPMAPMASK, R.IS_6_BIT_USEMIPMAPMASK_INVERSE):
        got = dec.decompress_alpha(mode, (bx, by, bw, bh), pay, mask, mbox)
        np.testing.assert_array_equal(got, R.decode(mode, (bx, by, bw, bh), pay, w, h, mask, mbox))


def test_gpu_decode_errors(dec):
    from yaik_amd._lib import YaikError
    w, h = 64, 48
    dec.begin(w, h)
    pay = np.zeros(w * h, np.uint8)
    for bbox in ((60, 0, 8, 8), (0, 44, 8, 8), (-8, 0, 8, 8), (0, 0, 0, 4), (64, 0, 8, 8)):
        with pytest.raises(YaikError):
            dec.decompress_alpha(R.IS_8_BIT_FULL, bbox, pay)
    with pytest.raises(YaikError):                     # payload shorter than the box needs
        dec.decompress_alpha(R.IS_8_BIT_FULL, (0, 0, 16, 16), pay[:255])
    with pytest.raises(YaikError):
        dec.decompress_alpha(R.IS_1_BIT_FULL, (0, 0, 16, 16), pay[:31])
    with pytest.raises(YaikError):
        dec.decompress_alpha(R.IS_6_BIT_FULL, (0, 0, 16, 16), pay[:191])
    with pytest.raises(YaikError):                     # 1-bit box width not a multiple of 8
        dec.decompress_alpha(R.IS_1_BIT_FULL, (0, 0, 12, 4), pay)
    for mode in (R.IS_1_BIT_USEMIPMAPMASK, 7):
        with pytest.raises(YaikError):
            dec.decompress_alpha(mode, (0, 0, 16, 16), pay)
    with pytest.raises(YaikError):                     # mask mode without a mask
        dec.decompress_alpha(R.IS_6_BIT_USEMIPMAPMASK, (0, 0, 16, 16), pay)
    mask = R.swizzled_mask(np.array([255], np.uint8), 1, 1)
    with pytest.raises(YaikError):                     # the mask selects 256 samples = 192 bytes
        dec.decompress_alpha(R.IS_6_BIT_USEMIPMAPMASK, (0, 0, 16, 16), pay[:191], mask, (0, 0, 16, 16))
    got = dec.decompress_alpha(R.IS_6_BIT_USEMIPMAPMASK, (0, 0, 16, 16), pay[:192], mask, (0, 0, 16, 16))
    assert got.shape == (h, w)


def test_gpu_image_uses_device_alpha(dec):
    w, h = 128, 64
    rng = np.random.default_rng(5)
    dec.begin(w, h)
    rgb = dec.image()
    pay = rng.integers(0, 256, 64 * 40, dtype=np.uint8)
    plane = dec.decompress_alpha(R.IS_8_BIT_FULL, (32, 8, 64, 40), pay)
    rgba = dec.image()
    assert rgba.shape == (h, w * 4)
    np.testing.assert_array_equal(rgba.reshape(h, w, 4)[..., 3], plane)
    np.testing.assert_array_equal(rgba.reshape(h, w, 4)[..., :3], rgb.reshape(h, w, 3))
    np.testing.assert_array_equal(rgba, dec.image(alpha=plane))
    dec.begin(w, h)                                    # a new image has no alpha plane until its 'ALPM' chunk
    assert dec.image().shape == (h, w * 3)


@pytest.mark.parametrize("mode", [R.IS_1_BIT_FULL, R.IS_6_BIT_FULL, R.IS_6_BIT_FULL_INVERSE, R.IS_8_BIT_FULL])
def test_gpu_decode_whole_image_box(dec, mode):
    """a box touching every edge of the image (the reference's 8-bit unpacker overflows there, so no fixture pins it)"""
    w, h = 80, 48
    rng = np.random.default_rng(40 + mode)
    n = {R.IS_8_BIT_FULL: w * h, R.IS_1_BIT_FULL: w // 8 * h}.get(mode, w // 4 * 3 * h)
    pay = rng.integers(0, 256, n, dtype=np.uint8)
    dec.begin(w, h)
    for quirk in ((False, True) if mode == R.IS_1_BIT_FULL else (False,)):
        np.testing.assert_array_equal(dec.decompress_alpha(mode, (0, 0, w, h), pay, reference_1bit=quirk),
                                      R.decode(mode, (0, 0, w, h), pay, w, h, reference_1bit=quirk))


# ---- encode: yk_alpha_values (EncoderContext::ProcessAlpha, force8Bit = true) ---------------------------------------------------------------
FORCE8 = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "alpha_*.npz"))) if int(np.load(p)["force8bit"])]


@pytest.fixture(scope="module")
def enc():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


def _planes(alpha, seed=7):
    h, w = alpha.shape
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 256, (h, w), dtype=np.int32) for _ in range(3)] + [alpha.astype(np.int32)])


def _gpu_encode(enc, alpha):
    enc.set_image(_planes(alpha))
    mp = enc.mip_prefilter()
    return mp, enc.alpha_values(True)


def _check_encode(enc, alpha):
    mp, got = _gpu_encode(enc, alpha)
    want = R.encode(alpha, mp["bounds"], None, True)    # force8Bit: the per-pixel mask is not read
    if want is None:
        assert got is None
    else:
        assert got is not None and got["mode"] == want["mode"] and got["bbox"] == tuple(want["bbox"])
        np.testing.assert_array_equal(got["payload"], want["payload"])
    return mp, got


@pytest.mark.parametrize("path", FORCE8, ids=lambda p: os.path.basename(p))
def test_gpu_encode_matches_fixture(enc, path):
    z = dict(np.load(path))
    mp, got = _check_encode(enc, z["alpha"])
    if np.array_equal(mp["bounds"], z["bounds"]):     # the search region is the same as the reference's: header and payload are too
        if not z["has_chunk"]:
            assert got is None
        else:
            hd = z["header"]
            assert got["mode"] == hd[7] and got["bbox"] == tuple(int(v) for v in hd[:4]) and len(got["payload"]) == hd[5]
            np.testing.assert_array_equal(got["payload"], z["payload"])


def _pattern(rng, h, w, kind):
    a = np.zeros((h, w), np.int32)
    y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
    y1, x1 = int(rng.integers(y0 + 1, h + 1)), int(rng.integers(x0 + 1, w + 1))
    if kind == "analog":
        a[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0))
    elif kind == "binary":
        a[y0:y1, x0:x1] = 255 * rng.integers(0, 2, (y1 - y0, x1 - x0))
    elif kind == "all255":
        a[:] = 255
    elif kind == "low":
        a[y0:y1, x0:x1] = rng.integers(0, 4, (y1 - y0, x1 - x0))
    elif kind == "low_edges":                          # binary inside, values 1..3 around it (inside the rounded box they make it analog)
        a[y0:y1, x0:x1] = rng.integers(1, 4, (y1 - y0, x1 - x0))
        a[(y0 + y1) // 2, (x0 + x1) // 2] = 255
    return a


@pytest.mark.parametrize("seed", range(12))
def test_gpu_encode_fuzz(enc, seed):
    rng = np.random.default_rng(2000 + seed)
    w, h = int(rng.integers(1, 24)) * 16, int(rng.integers(1, 24)) * 16
    for kind in ("analog", "binary", "all255", "low", "low_edges", "empty"):
        _check_encode(enc, _pattern(rng, h, w, kind))


@pytest.mark.parametrize("kind", ["analog", "binary"])
def test_gpu_encode_8192(enc, kind):
    rng = np.random.default_rng(8192 if kind == "analog" else 8193)
    w = h = 8192
    a = np.zeros((h, w), np.int32)
    a[1000:7001, 333:8000] = rng.integers(0, 256, (6001, 7667)) if kind == "analog" else 255 * rng.integers(0, 2, (6001, 7667))
    _check_encode(enc, a)


# ---- the C++ drop-in: ConvertHotPath with the 'ALPM' opt-in, YAIK_DecodeImage ----------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADRV = os.path.join(ROOT, "yaik_amd", "host", "alpha_driver")
TAG_ALPM = 0x4D504C41


@pytest.fixture(scope="module")
def adrv():
    import subprocess
    subprocess.run(["make", "-C", os.path.join(ROOT, "yaik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return ADRV


def _encode_file(adrv, planes, emit, tmp, parallel=False):
    import struct
    import subprocess
    n, h, w = planes.shape
    fin, fy = os.path.join(tmp, "in.bin"), os.path.join(tmp, f"out{int(emit)}{int(parallel)}.yaik")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", w, h, n)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())
    subprocess.run([adrv, "enc", fin, fy, "1" if emit else "0"] + (["parallel"] if parallel else []), check=True)
    with open(fy, "rb") as f:
        return f.read()


def _decode_file(adrv, data, tmp):
    import subprocess
    fi, fo = os.path.join(tmp, "d.yaik"), os.path.join(tmp, "d.out")
    with open(fi, "wb") as f:
        f.write(data)
    subprocess.run([adrv, "dec", fi, fo], check=True)
    raw = open(fo, "rb").read()
    res = np.frombuffer(raw[:40], np.int32)
    out = {"ok": int(res[0]), "err": int(res[1]), "w": int(res[2]), "h": int(res[3]), "bpp": int(res[5]), "custom_ok": int(res[6]),
           "custom_err": int(res[7]), "has_plane_a": int(res[8]), "stride_a": int(res[9])}
    p = 40
    if out["ok"]:
        n = out["w"] * out["h"] * out["bpp"]
        out["image"] = np.frombuffer(raw[p:p + n], np.uint8).reshape(out["h"], out["w"], out["bpp"]); p += n
    if out["has_plane_a"]:
        out["plane_a"] = np.frombuffer(raw[p:p + out["w"] * out["h"]], np.uint8).reshape(out["h"], out["w"])
    return out


def _chunks(data):
    """(offset, tag, length) of every chunk after the file header, up to the terminator"""
    import struct
    out, p = [], 12
    while p + 4 <= len(data):
        tag = struct.unpack_from("<I", data, p)[0]
        if tag == 0xDEADBEEF:
            break
        ln = struct.unpack_from("<I", data, p + 4)[0]
        out.append((p, tag, ln))
        p += 8 + ln
    return out


def _round_trip_alpha(kind, h=96, w=128):
    rng = np.random.default_rng(77)
    a = np.zeros((h, w), np.int32)
    a[10:70, 20:100] = rng.integers(0, 256, (60, 80)) if kind == "analog" else 255 * rng.integers(0, 2, (60, 80))
    a[10, 20] = 255
    return a


@pytest.mark.parametrize("kind", ["analog", "binary"])
def test_convert_hot_path_alpha_round_trip(adrv, tmp_path, kind):
    a = _round_trip_alpha(kind)
    planes = _planes(a)
    on = _encode_file(adrv, planes, True, str(tmp_path))
    off = _encode_file(adrv, planes, False, str(tmp_path))
    tags = [t for _, t, _ in _chunks(on)]
    assert TAG_ALPM in tags and TAG_ALPM not in [t for _, t, _ in _chunks(off)]
    assert tags.index(TAG_ALPM) == 1                   # right after 'MIPM'
    # the opt-in only inserts the chunk: without it the file is the one the drop-in always wrote
    p, _, ln = next(c for c in _chunks(on) if c[1] == TAG_ALPM)
    assert on[:p] + on[p + 8 + ln:] == off
    assert _encode_file(adrv, planes, True, str(tmp_path), parallel=True) == on
    d_on, d_off = _decode_file(adrv, on, str(tmp_path)), _decode_file(adrv, off, str(tmp_path))
    assert d_on["ok"] and d_off["ok"] and d_on["bpp"] == 4 and d_off["bpp"] == 3
    np.testing.assert_array_equal(d_on["image"][..., 3], a.astype(np.uint8))   # 8-bit exact; binary exactly 0 / 255
    np.testing.assert_array_equal(d_on["image"][..., :3], d_off["image"])
    assert d_on["custom_ok"] and d_on["has_plane_a"] and d_on["stride_a"] == a.shape[1]
    np.testing.assert_array_equal(d_on["plane_a"], a.astype(np.uint8))
    assert d_off["custom_ok"] and not d_off["has_plane_a"]


def test_convert_hot_path_option_off_is_unchanged(adrv, tmp_path):
    """with the opt-in off the drop-in writes exactly what ConvertHotPath always wrote (host_driver's stream of the same image)"""
    import struct
    import subprocess
    a = _round_trip_alpha("analog")
    planes = _planes(a)
    off = _encode_file(adrv, planes, False, str(tmp_path))
    fin, fb, fy = str(tmp_path / "h.bin"), str(tmp_path / "h.blobs"), str(tmp_path / "h.yaik")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", 128, 96, 4)); f.write(planes.tobytes())
    subprocess.run([os.path.join(ROOT, "yaik_amd", "host", "host_driver"), fin, fb, "0", fy], check=True, stdout=subprocess.DEVNULL)
    assert open(fy, "rb").read() == off


def _patched(data, **fields):
    """the file with fields of its 'ALPM' AlphaHeader replaced (bbox x, y, w, h: s16; expected: u32; parameters: u8)"""
    import struct
    b = bytearray(data)
    p, _, _ = next(c for c in _chunks(data) if c[1] == TAG_ALPM)
    h = p + 8
    if "bbox" in fields:
        struct.pack_into("<4h", b, h, *fields["bbox"])
    if "expected" in fields:
        struct.pack_into("<I", b, h + 12, fields["expected"])
    if "parameters" in fields:
        b[h + 17] = fields["parameters"]
    return bytes(b)


YAIK_INVALID_STREAM, YAIK_INVALID_DECOMPRESSION = 6, 13
YAIK_ALPHA_FORMAT_IMPOSSIBLE, YAIK_INVALID_ALPHA_FORMAT, YAIK_ALPHA_UNSUPPORTED_YET = 17, 18, 19


def test_decode_image_alpha_error_codes(adrv, tmp_path):
    a = _round_trip_alpha("analog")
    on = _encode_file(adrv, _planes(a), True, str(tmp_path))
    assert [t for _, t, _ in _chunks(on)][0] == 0x4D50494D     # 'MIPM' first: the 'ALPM' chunk is read at state 1
    cases = [(dict(parameters=0), YAIK_ALPHA_UNSUPPORTED_YET), (dict(parameters=7), YAIK_INVALID_ALPHA_FORMAT),
             (dict(bbox=(120, 10, 16, 60)), YAIK_INVALID_STREAM), (dict(bbox=(-4, 10, 80, 60)), YAIK_INVALID_STREAM),
             (dict(bbox=(20, 10, 80, 90)), YAIK_INVALID_STREAM)]
    x, y, bw, bh = 20, 10, 80, 60
    cases.append((dict(expected=bw * bh + 1), YAIK_INVALID_DECOMPRESSION))      # the stream is shorter than the header claims
    for f, code in cases:
        d = _decode_file(adrv, _patched(on, **f), str(tmp_path))
        assert not d["ok"] and d["err"] == code, (f, d["err"])
    # state 0 (no 'MIPM': the kept tiles span the image): the mask modes are impossible there
    full = _planes(np.full((64, 64), 128, np.int32))
    f0 = _encode_file(adrv, full, True, str(tmp_path))
    assert [t for _, t, _ in _chunks(f0)][0] == TAG_ALPM
    for m in (0, 2, 3):
        d = _decode_file(adrv, _patched(f0, parameters=m), str(tmp_path))
        assert not d["ok"] and d["err"] == YAIK_ALPHA_FORMAT_IMPOSSIBLE, (m, d["err"])
    assert _decode_file(adrv, f0, str(tmp_path))["ok"]
