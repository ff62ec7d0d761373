"""Decode of images whose width and/or height is 8 (mod 16), on the GPU: every decode entry point against the CPU oracle's consistent reading
(DESIGN §10), chunk by chunk and end to end through the YAIK_* API; tiles that reach past the right edge are skipped without consuming
anything; sides that are not multiples of 8 are still refused."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import PASSES, OracleDecoder, OracleEncoder, dec_mask, detile, image_builder, palette_remap
from tests import alpha_ref as R
from tests.ragged import LARGE, SHAPES, oracle_streams, psnr, source, stream_lengths_1d

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
DRIVER = os.path.join(HOST, "host_driver")
ADRV = os.path.join(HOST, "alpha_driver")
YAIK_INVALID_HEADER = 7


@pytest.fixture(scope="module")
def dec():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def hip():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def drivers(oracle_built):
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    return True


def _gradients(dec, od, passes):
    for sx, sy, cnt, bm, rgb in passes:
        if cnt:
            od.gradient(sx, sy, bm, rgb)
            dec.decompress_gradient(sx, sy, bm, rgb)


@pytest.mark.parametrize("w,h,kind", SHAPES + LARGE)
def test_chunks_match_oracle(dec, oracle_built, w, h, kind):
    planes = source(w, h, kind)
    passes, typ, pix = oracle_streams(planes)
    od = OracleDecoder(w, h)
    dec.begin(w, h)
    _gradients(dec, od, passes)
    assert np.array_equal(dec.planes(), od.planes()), "gradient fill differs"
    t4 = dec.tile4x4()
    assert np.array_equal(t4, od.tile4x4()), "tile4x4Mask differs"
    # the 1-D pass walks the w/8 x h/8 tiles: the cursors end exactly at the ends of both streams
    assert stream_lengths_1d(t4, w, h) == (typ.size, pix.size)
    od.split_masks()
    assert od.decode_1d(typ, pix) == (typ.size, pix.size)
    dec.decompress_1d(typ, pix)
    gp = dec.planes()
    assert np.array_equal(gp, od.planes()), "1-D range fill differs"
    rec = np.stack([detile(gp[c], w, h) for c in range(3)])
    assert psnr(rec, planes[:3]) > 30.0
    # nothing past the stream ends is read: trailing bytes change nothing
    if w * h <= 1 << 22:
        dec.begin(w, h)
        _gradients(dec, OracleDecoder(w, h), passes)
        dec.decompress_1d(np.concatenate([typ, np.full(64, 0xFF, np.uint8)]), np.concatenate([pix, np.full(64, 0xFF, np.uint8)]))
        assert np.array_equal(dec.planes(), gp)
    # default image builder: RGB, the documented RGBA layout, the reference's RGBA branch; padded strides keep their padding
    want = np.stack([detile(gp[c], w, h) for c in range(3)], axis=-1).reshape(h, w * 3)
    img = dec.image(stride=w * 3 + 13, fill=0xA5)
    assert np.array_equal(img, image_builder(gp, w, h, w * 3 + 13))
    assert np.array_equal(img[:, : w * 3], want) and (img[:, w * 3:] == 0xA5).all()
    alpha = (np.arange(h * w, dtype=np.int64).reshape(h, w) % 251).astype(np.uint8)
    rgba = dec.image(alpha=alpha, stride=w * 4 + 8, fill=0x5A)
    assert (rgba[:, w * 4:] == 0x5A).all()
    rgba = rgba[:, : w * 4].reshape(h, w, 4)
    assert np.array_equal(rgba[..., :3], want.reshape(h, w, 3)) and np.array_equal(rgba[..., 3], alpha)
    ref_rgba = dec.image(alpha=alpha, stride=w * 4 + 20, fill=0xA5, reference_rgba=True)
    assert np.array_equal(ref_rgba, image_builder(gp, w, h, w * 4 + 20, alpha=alpha))


@pytest.mark.parametrize("w,h,kind", SHAPES + LARGE)
def test_device_streams_equal_host_streams(hip, w, h, kind):
    from yaik_amd.decoder import HipTileDecoder
    planes = source(w, h, kind)
    hip.set_image(planes)
    hip.encode(3, False, False)
    counts = hip.gradient_counts()
    a, b = HipTileDecoder(0), HipTileDecoder(0)
    try:
        a.begin(w, h)
        for i, (sx, sy) in enumerate(PASSES):
            if counts[i]:
                a.decompress_gradient(sx, sy, hip.gradient_bitmap(i), palette_remap(hip.gradient_corners(i), 250))
        pix, typ = hip.dynamic_tile_compressor()
        a.decompress_1d(typ, pix)
        want, want4 = a.planes(), a.tile4x4()
        for per_pass in (False, True):
            b.begin(w, h)
            b.decode_from_encoder(hip, per_pass=per_pass)
            assert np.array_equal(b.planes(), want), per_pass
            assert np.array_equal(b.tile4x4(), want4), per_pass
    finally:
        a.close(); b.close()


def test_plane_subset_passes_match_oracle(dec, oracle_built):
    from tests.blobs import PP_MASKS
    from tests.images import edge_image
    w, h = 200, 72
    planes = edge_image(w, h, "planemix", 3)
    ora = OracleEncoder(planes)
    od = OracleDecoder(w, h)
    dec.begin(w, h)
    for sx, sy in PASSES:
        cnt, bm, rgb = ora.fitting_quad_smooth(sx, sy)
        if cnt:
            dq = palette_remap(rgb, 250)
            od.gradient(sx, sy, bm, dq); dec.decompress_gradient(sx, sy, bm, dq)
    od.split_masks()
    done = 0
    for m in PP_MASKS:
        cnt, bm, rgb = ora.fitting_quad_smooth(2, 2, plane_bit=m)
        if cnt:
            dq = palette_remap(rgb, 250)
            od.gradient_planes(m, bm, dq, consistent_marks=True)
            dec.decompress_gradient_planes(m, bm, dq, consistent_marks=True)
            done += 1
    assert done > 0
    assert np.array_equal(dec.planes(), od.planes())
    assert np.array_equal(dec.tile4x4(all_planes=True), od.tile4x4(all_planes=True))
    for p in range(3):
        ora.dynamic_tile_compressor(p)
    pix, typ = ora.streams_1d()
    assert od.decode_1d(typ, pix) == (typ.size, pix.size)
    dec.decompress_1d(typ, pix)
    assert np.array_equal(dec.planes(), od.planes())


def _slot(sx, sy, w, bx, by):
    """bit index of the first tile slot of swizzle block (bx, by) of a tile map of 2^sx x 2^sy tiles"""
    bigX, bigY = (32 if sx == 2 else 64), (32 if sy == 2 else 64)
    return (by * ((w + bigX - 1) // bigX) + bx) * (bigX >> sx) * (bigY >> sy)


def _set_bit(bm, pos):
    out = np.array(bm, dtype=np.uint8, copy=True)
    out[pos >> 3] |= np.uint8(1 << (pos & 7))
    return out


def test_gradient_tile_across_the_right_edge_is_skipped(dec, oracle_built):
    """A 16x16 tile at x = w - 8: no encoder writes it, a stream can hold it.  It is skipped before its corners are counted, in the per-pass
    kernels and in the all-pass kernels (owner, stream count / emit, block render), so the decode equals the decode without the bit, as in
    the oracle."""
    import ctypes as C
    import torch
    from yaik_amd._lib import lib
    from yaik_amd.decoder import HipTileDecoder
    from yaik_amd.encoder import _chk
    w, h = 200, 72
    planes = source(w, h, "photo")
    passes, typ, pix = oracle_streams(planes)
    pos = _slot(4, 4, w, w // 64, 0)                                  # the 16x16 tile at x = 192 reaches to 208 > w
    sx0, sy0, cnt0, bm0, rgb0 = passes[0]
    assert not (bm0[pos >> 3] >> (pos & 7)) & 1
    crossed = [(sx0, sy0, cnt0 + 1, _set_bit(bm0, pos), rgb0)] + passes[1:]
    od, ox = OracleDecoder(w, h), OracleDecoder(w, h)
    dec.begin(w, h)
    _gradients(dec, od, passes)
    want, want4 = dec.planes(), dec.tile4x4()
    dec.begin(w, h)
    _gradients(dec, ox, crossed)
    assert np.array_equal(od.planes(), ox.planes()) and np.array_equal(od.planes(), want)
    assert np.array_equal(dec.planes(), want) and np.array_equal(dec.tile4x4(), want4)
    # the same streams from device memory: one yk_decode_gradient_all_device call, and one yk_decode_gradient_device call per pass
    g = [p for p in crossed if p[2]]
    dev_b = [torch.from_numpy(np.ascontiguousarray(p[3])).cuda() for p in g]
    dev_r = [torch.from_numpy(np.concatenate([p[4], np.zeros(1, np.uint8)])).cuda() for p in g]
    torch.cuda.synchronize()
    b = HipTileDecoder(0)
    try:
        n = len(g)
        sx = (C.c_int * n)(*[p[0] for p in g]); sy = (C.c_int * n)(*[p[1] for p in g])
        bm = (C.c_void_p * n)(*[t.data_ptr() for t in dev_b]); nb = (C.c_size_t * n)(*[p[3].size for p in g])
        rp = (C.c_void_p * n)(*[t.data_ptr() for t in dev_r]); nr = (C.c_size_t * n)(*[p[4].size for p in g])
        b.begin(w, h)
        _chk(b._h, lib().yk_decode_gradient_all_device(b._h, n, sx, sy, bm, nb, rp, nr, 0))
        b.synchronize()
        assert np.array_equal(b.planes(), want) and np.array_equal(b.tile4x4(), want4)
        b.begin(w, h)
        for k in range(n):
            _chk(b._h, lib().yk_decode_gradient_device(b._h, sx[k], sy[k], bm[k], nb[k], rp[k], nr[k], 0))
        b.synchronize()
        assert np.array_equal(b.planes(), want) and np.array_equal(b.tile4x4(), want4)
    finally:
        b.close()


def _lut_case(hip, w, h, seed):
    from oracle.pyoracle import yko_compress_f
    from tests.blobs import LUT_PASSES
    from tests.lutbank import bank_patterns, lut_image
    pats = bank_patterns()
    planes = lut_image(w, h, pats, seed)
    ora = OracleEncoder(planes)
    hip.lut_clear()
    for p in pats:
        hip.lut_load(p); ora.lut_load(p)
    hip.set_image(planes)
    hip.encode(3, False, False)
    grads = []
    for i, (sx, sy) in enumerate(PASSES):
        bm, rgb = hip.gradient_bitmap(i), hip.gradient_corners(i)
        if rgb.size:
            grads.append((sx, sy, 1, bm, palette_remap(rgb, 250)))
    hip.lut_start()
    for sx, sy in LUT_PASSES:
        hip.lut_search(sx, sy)
    s = hip.lut_streams()
    colors = palette_remap(yko_compress_f(s["color"], 250), 250)
    idx = [(s[f"idx{b}"].astype(np.uint16) * 3).astype(np.uint8) for b in (3, 4, 5, 6)]
    maps = [np.array(s[f"map{k}"], np.uint8) for k in range(6)]
    pix, typ = hip.dynamic_tile_compressor()
    hip.lut_clear()
    return planes, ora.lut_file(), grads, maps, s["tileType"], colors, idx, typ, pix


def test_lut3d_matches_oracle_and_skips_tiles_across_the_edges(hip, dec, oracle_built):
    w, h = 200, 136
    planes, lut_file, grads, maps, tiles, colors, idx, typ, pix = _lut_case(hip, w, h, 5)
    assert tiles.size > 0
    od = OracleDecoder(w, h)
    dec.begin(w, h)
    _gradients(dec, od, grads)
    want_used = od.lut3d(lut_file, maps, tiles, colors, idx)
    dec.assign_lut(lut_file)
    used = dec.decompress_lut3d(maps, tiles, colors, idx)
    assert used.tolist() == want_used.tolist() == [tiles.size * 2, colors.size] + [i.size for i in idx]
    assert np.array_equal(dec.planes(), od.planes()) and np.array_equal(dec.tile4x4().ravel(), od.tile4x4().ravel())
    want, want4 = dec.planes(), dec.tile4x4()
    od.split_masks()
    assert od.decode_1d(typ, pix) == (typ.size, pix.size)
    dec.decompress_1d(typ, pix)
    assert np.array_equal(dec.planes(), od.planes())
    # a 16x8 tile across the right edge (map 0) and an 8x16 tile across the bottom edge (map 1): skipped, nothing consumed (the project's
    # rule; the encoder never writes such tiles)
    crossed = list(maps)
    p0 = _slot(4, 3, w, w // 64, 0)                                   # 16x8 at x = 192 .. 207, w = 200
    p1 = _slot(3, 4, w, 0, h // 64)                                   # 8x16 at y = 128 .. 143, h = 136
    for k, p in ((0, p0), (1, p1)):
        assert crossed[k].size * 8 > p and not (crossed[k][p >> 3] >> (p & 7)) & 1
        crossed[k] = _set_bit(crossed[k], p)
    dec.begin(w, h)
    _gradients(dec, OracleDecoder(w, h), grads)
    assert dec.decompress_lut3d(crossed, tiles, colors, idx).tolist() == used.tolist()
    assert np.array_equal(dec.planes(), want) and np.array_equal(dec.tile4x4(), want4)


RGBA_SHAPES = [(24, 40), (200, 72), (136, 264), (1080, 1920)]


@pytest.mark.parametrize("w,h", RGBA_SHAPES)
def test_mask_and_alpha_unpackers(dec, oracle_built, w, h):
    rng = np.random.default_rng(w * 3 + h)
    dec.begin(w, h)
    rgb = dec.image()                                                 # the RGB rows before any alpha plane exists
    # 'MIPM': the tile box covers the clipped 16x16 edge tiles
    tbw, tbh = (w + 15) // 16, (h + 15) // 16
    bits = rng.integers(0, 256, (tbw * tbh + 7) // 8, dtype=np.uint8)
    mask = dec.decompress_1bit_tiled(bits, tbw, tbh)
    assert np.array_equal(mask, dec_mask(bits, tbw, tbh))
    for mode in (R.IS_1_BIT_FULL, R.IS_6_BIT_FULL, R.IS_6_BIT_FULL_INVERSE, R.IS_8_BIT_FULL):
        for whole in (True, False):
            if whole:
                bw, bh, bx, by = w, h, 0, 0
            else:
                bw = int(rng.integers(1, w // 8 + 1)) * 8
                bh = int(rng.integers(1, h + 1))
                bx = int(rng.integers(0, (w - bw) // 8 + 1)) * 8
                by = int(rng.integers(0, h - bh + 1))
            n = bw * bh if mode == R.IS_8_BIT_FULL else bw // 8 * bh if mode == R.IS_1_BIT_FULL else bw // 4 * 3 * bh
            pay = rng.integers(0, 256, n, dtype=np.uint8)
            for quirk in ((False, True) if mode == R.IS_1_BIT_FULL and bw > 8 else (False,)):
                got = dec.decompress_alpha(mode, (bx, by, bw, bh), pay, reference_1bit=quirk)
                np.testing.assert_array_equal(got, R.decode(mode, (bx, by, bw, bh), pay, w, h, reference_1bit=quirk))
            out = dec.image().reshape(h, w, 4)                     # RGBA rows from the plane kept on the device
            assert np.array_equal(out[..., :3], rgb.reshape(h, w, 3)) and np.array_equal(out[..., 3], got)
    # mask modes over the whole tile box, clipped right / bottom tiles included: the alpha box reaches the image edges
    mbox = (0, 0, tbw * 16, tbh * 16)
    for bx, by, bw, bh in ((0, 0, w, h), (w - 8 - 4 * int(rng.integers(0, w // 8)), h // 2, 8, h - h // 2)):
        bw = bw if bx + bw <= w else w - bx
        pay = rng.integers(0, 256, bw * bh, dtype=np.uint8)
        for mode in (R.IS_6_BIT_USEMIPMAPMASK, R.IS_6_BIT_USEMIPMAPMASK_INVERSE):
            got = dec.decompress_alpha(mode, (bx, by, bw, bh), pay, mask, mbox)
            np.testing.assert_array_equal(got, R.decode(mode, (bx, by, bw, bh), pay, w, h, mask, mbox))


# ---- end to end through the C++ mirror and the YAIK_* API ----------------------------------------------------------------------------
def _write_in(path, planes):
    n, h, w = planes.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", w, h, n)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())


def _host_round_trip(planes, tmp):
    from oracle.refrun import parse_blobs
    fin, fout, fy = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.blobs"), os.path.join(tmp, "out.yaik")
    _write_in(fin, planes)
    subprocess.run([DRIVER, fin, fout, "0", fy], check=True, stdout=subprocess.DEVNULL)
    return parse_blobs(fout)


def _alpha_encode(planes, tmp, emit, *opts):
    fin, fy = os.path.join(tmp, "ain.bin"), os.path.join(tmp, "a.yaik")
    _write_in(fin, planes)
    subprocess.run([ADRV, "enc", fin, fy, "1" if emit else "0", *opts], check=True)
    return open(fy, "rb").read()


def _alpha_decode(data, tmp):
    fi, fo = os.path.join(tmp, "d.yaik"), os.path.join(tmp, "d.out")
    with open(fi, "wb") as f:
        f.write(data)
    subprocess.run([ADRV, "dec", fi, fo], check=True)
    raw = open(fo, "rb").read()
    res = np.frombuffer(raw[:40], np.int32)
    out = {"ok": int(res[0]), "err": int(res[1]), "w": int(res[2]), "h": int(res[3]), "bpp": int(res[5]), "custom_ok": int(res[6]),
           "has_plane_a": int(res[8]), "stride_a": int(res[9])}
    p = 40
    if out["ok"]:
        n = out["w"] * out["h"] * out["bpp"]
        out["image"] = np.frombuffer(raw[p:p + n], np.uint8).reshape(out["h"], out["w"], out["bpp"]); p += n
    if out["has_plane_a"]:
        out["plane_a"] = np.frombuffer(raw[p:p + out["w"] * out["h"]], np.uint8).reshape(out["h"], out["w"])
    return out


def _gpu_chunk_decode(data, w, h):
    """the GPU decode of a .yaik file's own 'GTIL' and '1DTL' chunks, one HipTileDecoder call per chunk (streams as the product's parser
    expands them: ZStd, then PaletteDecompressor): tiled planes and RGB rows"""
    from tests import chunks
    from yaik_amd.decoder import HipTileDecoder
    c = chunks.parse(data, w, h)
    n = int(np.frombuffer(c["chunk_count_terminated"], np.int32)[0])
    d = HipTileDecoder(0)
    try:
        d.begin(w, h)
        for i in range(n):
            if c[f"c{i}_tag"] == b"GTIL":
                fmt = int(np.frombuffer(c[f"c{i}_hdr"], np.int32)[7])          # the parser's header fields: ..., colorCompression, format, plane
                d.decompress_gradient(fmt & 7, (fmt >> 3) & 7, np.frombuffer(c[f"c{i}_bitmap"], np.uint8), np.frombuffer(c[f"c{i}_rgb"], np.uint8))
            elif c[f"c{i}_tag"] == b"1DTL":
                d.decompress_1d(np.frombuffer(c[f"c{i}_type"], np.uint8), np.frombuffer(c[f"c{i}_pix"], np.uint8),
                               int(np.frombuffer(c[f"c{i}_hdr"], np.int32)[3]))          # ..., compressionColor, compressionRange, version
        return d.planes(), d.image().reshape(h, w, 3)
    finally:
        d.close()


@pytest.mark.parametrize("w,h,kind", [(200, 72, "photo"), (1920, 1080, "photo")])
def test_convert_then_decode_image_rgb(drivers, tmp_path, w, h, kind):
    from tests import chunks
    planes = source(w, h, kind)
    got = _host_round_trip(planes, str(tmp_path))
    s = chunks.oracle_streams(planes)
    for k in [k for k in s if k.startswith("plnt_")]:
        del s[k]
    bad = chunks.compare_parsed(chunks.parse(chunks.frame(s, with_file_header=True), w, h), chunks.parse(got["yaik_file"], w, h))
    assert not bad, bad
    tiled, img = _gpu_chunk_decode(got["yaik_file"], w, h)
    assert np.frombuffer(got["yaik_dims"], np.int32).tolist() == [w, h, 3]
    assert got["yaik_planes_tiled"] == tiled.tobytes()
    rows = np.frombuffer(got["yaik_image"], np.uint8).reshape(h, w, 3)
    assert np.array_equal(rows, img)
    p = psnr(np.moveaxis(rows, -1, 0), planes[:3])
    assert p > 30.0, p


def _rgba(w, h, seed):
    rng = np.random.default_rng(seed)
    rgb = source(w, h, "photo")
    a = np.zeros((h, w), np.int32)
    a[16:h, 32:w] = rng.integers(0, 256, (h - 16, w - 32))        # the box reaches the clipped right / bottom tiles
    a[16, 32] = a[h - 1, w - 1] = 200
    return np.concatenate([rgb, a[None]]), a


@pytest.mark.parametrize("w,h", [(200, 72), (1080, 1920)])
def test_convert_then_decode_image_rgba(drivers, tmp_path, w, h):
    planes, a = _rgba(w, h, w + h)
    on = _alpha_encode(planes, str(tmp_path), True)
    off = _alpha_encode(planes, str(tmp_path), False)
    d_on, d_off = _alpha_decode(on, str(tmp_path)), _alpha_decode(off, str(tmp_path))
    assert d_on["ok"] and d_off["ok"] and d_on["bpp"] == 4 and d_off["bpp"] == 3
    np.testing.assert_array_equal(d_on["image"][..., 3], a.astype(np.uint8))
    np.testing.assert_array_equal(d_on["image"][..., :3], d_off["image"])
    assert d_on["custom_ok"] and d_on["has_plane_a"] and d_on["stride_a"] == w
    np.testing.assert_array_equal(d_on["plane_a"], a.astype(np.uint8))
    _, img = _gpu_chunk_decode(off, w, h)
    assert np.array_equal(d_off["image"], img)
    p = psnr(np.moveaxis(d_on["image"][..., :3], -1, 0), planes[:3])
    assert p > 30.0, p
    # 6-bit mask mode: every tile of the 'MIPM' box is kept, clipped edge tiles included
    six = _alpha_encode(planes, str(tmp_path), True, "alpha6")
    d6 = _alpha_decode(six, str(tmp_path))
    assert d6["ok"] and d6["bpp"] == 4
    want = np.zeros((h, w), np.uint8)
    v = a[16:h, 32:w]
    want[16:h, 32:w] = ((v >> 2) << 2) | (v >> 6)
    want[a >> 2 == 0] = 0
    np.testing.assert_array_equal(d6["image"][..., 3], want)
    np.testing.assert_array_equal(d6["image"][..., :3], d_off["image"])


def test_one_handle_and_one_slot_decode_three_sizes(drivers, tmp_path):
    from oracle.refrun import parse_blobs
    from yaik_amd.decoder import HipTileDecoder
    # one HipTileDecoder handle
    d = HipTileDecoder(0)
    try:
        for w, h in ((1920, 1080), (1024, 1024), (1080, 1920), (1920, 1080)):
            planes = source(w, h, "photo")
            passes, typ, pix = oracle_streams(planes)
            od = OracleDecoder(w, h)
            d.begin(w, h)
            _gradients(d, od, passes)
            od.split_masks(); od.decode_1d(typ, pix)
            d.decompress_1d(typ, pix)
            assert np.array_equal(d.planes(), od.planes()), (w, h)
            assert np.array_equal(d.image().reshape(h, w, 3), np.stack([detile(od.planes()[c], w, h) for c in range(3)], axis=-1)), (w, h)
    finally:
        d.close()
    # one YAIK decode slot: three files of different sizes decoded in turn
    files, want = [], []
    for i, (w, h) in enumerate(((1920, 1080), (1024, 1024))):
        got = _host_round_trip(source(w, h, "smooth"), str(tmp_path))
        path = os.path.join(str(tmp_path), f"f{i}.yaik")
        with open(path, "wb") as f:
            f.write(got["yaik_file"])
        files.append(path); want.append(np.frombuffer(got["yaik_image"], np.uint8))
    planes, a = _rgba(1080, 1920, 9)
    data = _alpha_encode(planes, str(tmp_path), True)
    path = os.path.join(str(tmp_path), "f2.yaik")
    with open(path, "wb") as f:
        f.write(data)
    files.append(path); want.append(_alpha_decode(data, str(tmp_path))["image"].ravel())
    out = os.path.join(str(tmp_path), "seq.blobs")
    subprocess.run([DRIVER, "decode", out] + files, check=True, stdout=subprocess.DEVNULL)
    got = parse_blobs(out)
    for i, (w, h, bpp) in enumerate(((1920, 1080, 3), (1024, 1024, 3), (1080, 1920, 4))):
        assert np.frombuffer(got[f"seq_info_{i}"], np.int32).tolist() == [1, 0, w, h, bpp], i
        assert np.array_equal(np.frombuffer(got[f"seq_image_{i}"], np.uint8), want[i]), i
    # sides that are not multiples of 8 are still refused: the header of the first file with width 1921
    bad = bytearray(open(files[0], "rb").read())
    assert struct.unpack_from("<HH", bad, 6) == (1920, 1080)
    struct.pack_into("<H", bad, 6, 1921)
    r = _alpha_decode(bytes(bad), str(tmp_path))
    assert not r["ok"] and r["err"] == YAIK_INVALID_HEADER


def test_begin_refuses_sides_that_are_not_multiples_of_8(dec):
    from yaik_amd._lib import YaikError
    for w, h in ((1920, 1084), (1921, 1080), (4, 8), (8, 32768)):
        with pytest.raises(YaikError):
            dec.begin(w, h)
    dec.begin(8, 8)
    dec.begin(32760, 72)
