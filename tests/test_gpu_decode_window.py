"""Window decode on the GPU (yk_decode_set_window): with a window set, image_window_device equals the crop of the whole decode, bit
for bit -- against the oracle's whole decode on the images and windows of tests/window_cases.py through both gradient paths, against a whole GPU
decode on encoder streams at 2048 x 2048 and on .yaik files -- tile4x4Mask stays whole, the planes outside the window's 64-blocks are not
written, and the calls that need the whole image refuse while a window is set."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import window_cases as WC

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_STAGE_DEC_DETILE = -2, -4, 5
TAG_GTIL = 0x4C495447


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dec2():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


_DEVICE_STREAMS = {}


def _device_calls(ref, key):
    """the oracle's streams of `ref` in device memory, as the call list of decode_streams (uploaded once per image, kept alive here)"""
    torch = _torch()
    if key not in _DEVICE_STREAMS:
        keep, calls = [], []
        for sx, sy, cnt, bm, rgb in ref.passes:
            if cnt:
                tb = torch.from_numpy(np.ascontiguousarray(bm)).cuda()
                tr = torch.from_numpy(np.concatenate([rgb, np.zeros(1, np.uint8)])).cuda()
                keep += [tb, tr]
                calls.append(("g", sx, sy, tb.data_ptr(), bm.size, tr.data_ptr(), rgb.size))
        tt, tp = torch.from_numpy(np.ascontiguousarray(ref.typ)).cuda(), torch.from_numpy(np.ascontiguousarray(ref.pix)).cuda()
        keep += [tt, tp]
        calls.append(("1", tt.data_ptr(), ref.typ.size, tp.data_ptr(), ref.pix.size))
        torch.cuda.synchronize()
        _DEVICE_STREAMS[key] = (keep, calls)
    return _DEVICE_STREAMS[key][1]


def _decode(d, ref, key, path, gradients_only=False):
    """the chunks of `ref` on handle d: "per_pass" = decompress_gradient per pass + decompress_1d on host streams (yk_dec_render_kernel),
    "all_pass" = decode_streams on uploaded streams with remap_range=0 (yk_decall_render_blocks_kernel)"""
    if path == "per_pass":
        for sx, sy, cnt, bm, rgb in ref.passes:
            if cnt:
                d.decompress_gradient(sx, sy, bm, rgb)
        if not gradients_only:
            d.decompress_1d(ref.typ, ref.pix)
    else:
        calls = _device_calls(ref, key)
        d.decode_streams([c for c in calls if c[0] == "g" or not gradients_only], remap_range=0)


def _refs(w, h, kind, second=False):
    return WC.reference(w, h, kind, second), (w, h, kind, second)


# ---- oracle streams: every case and window, both gradient paths ----------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["per_pass", "all_pass"])
@pytest.mark.parametrize("w,h,kind,win", WC.all_case_windows(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_window_equals_the_oracle_crop(dec, oracle_built, w, h, kind, win, path):
    ref, key = _refs(w, h, kind)
    dec.begin(w, h)
    assert dec.window is None
    dec.set_window(*win)
    assert dec.window == win
    _decode(dec, ref, key, path)
    got = dec.image_window_device()
    assert tuple(got.shape) == (win[3], win[2], 3)
    assert np.array_equal(got.cpu().numpy(), ref.crop(win))
    # the marks are whole-image and exact: the 1-D count and scan read them for every tile
    assert np.array_equal(dec.tile4x4(), ref.tile4)
    # the planes are exact inside the window
    x0, y0, ww, wh = win
    inside = np.s_[:, y0 // 8:(y0 + wh) // 8, x0 // 8:(x0 + ww) // 8]
    assert np.array_equal(WC.tiles_of(dec.planes(), w, h)[inside], WC.tiles_of(ref.planes, w, h)[inside])


def _alpha_plane(d, w, h, seed):
    """an 8-bit 'ALPM' plane decoded on d (mode 6, a box that leaves the first 8 rows and columns out); returns the plane [h, w] as the library holds it"""
    rng = np.random.default_rng(seed)
    bx, by, bw, bh = (8, 8, w - 8, h - 8) if w > 16 and h > 16 else (0, 0, w, h)
    return d.decompress_alpha(6, (bx, by, bw, bh), rng.integers(1, 256, bw * bh).astype(np.uint8))


def _padded(torch, shape, planar, pad):
    """a sentinel-filled buffer and a view of it with row (and plane) padding, at an odd offset; returns buf, view, and the same pair in numpy"""
    if planar:
        c, hh, ww = shape
        row, off = ww + pad, 3
        plane = row * hh + 13
        n = off + c * plane + 64
        strides = (plane, row, 1)
    else:
        hh, ww, c = shape
        row, off = ww * c + pad, 5
        n = off + row * hh + 64
        strides = (row, c, 1)
    buf = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, shape, strides, off)
    nbuf = np.full(n, SENTINEL, np.uint8)
    nview = np.lib.stride_tricks.as_strided(nbuf[off:], shape, strides)
    return buf, view, nbuf, nview


@pytest.mark.parametrize("path", ["per_pass", "all_pass"])
@pytest.mark.parametrize("w,h,kind,win", [(520, 264, "mixed", WC.SCAN_BLOCK_WINDOW), (136, 264, "mixed", (128, 256, 8, 8)), (136, 264, "mixed", (64, 0, 8, 264)),
                                          (264, 136, "photo", (0, 64, 264, 8))])
def test_layouts_alpha_and_padding(dec, oracle_built, w, h, kind, win, path):
    torch = _torch()
    ref, key = _refs(w, h, kind)
    x0, y0, ww, wh = win
    dec.begin(w, h)
    dec.set_window(*win)
    alpha = _alpha_plane(dec, w, h, seed=w + h)                              # the plane stays whole; the window reads it at its offset
    assert alpha.shape == (h, w) and alpha[y0:y0 + wh, x0:x0 + ww].any()
    _decode(dec, ref, key, path)
    rgb, a_crop = ref.crop(win), alpha[y0:y0 + wh, x0:x0 + ww]
    for channels, a_arg, a_want in ((3, None, None), (4, None, a_crop), (4, 77, np.full((wh, ww), 77, np.uint8)), (None, None, a_crop)):
        want = rgb if a_want is None else np.concatenate([rgb, a_want[..., None]], axis=2)
        for planar in (False, True):
            exp = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
            got = dec.image_window_device(channels=channels, alpha=a_arg, planar=planar)
            assert np.array_equal(got.cpu().numpy(), exp), (channels, a_arg, planar)
            buf, view, nbuf, nview = _padded(torch, exp.shape, planar, pad=11)
            out = dec.image_window_device(out=view, channels=channels, alpha=a_arg, planar=planar)
            assert out is view
            nview[...] = exp
            assert np.array_equal(buf.cpu().numpy(), nbuf), (channels, a_arg, planar)      # nothing outside the pixel bytes changed
    with pytest.raises(ValueError, match="window"):
        dec.image_window_device(out=torch.empty((wh + 8, ww, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="window"):
        dec.image_window_device(out=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"))


# ---- work is skipped: nothing outside the window's 64-blocks is written --------------------------------------------------------------------
@pytest.mark.parametrize("path", ["per_pass", "all_pass"])
@pytest.mark.parametrize("win", [WC.SCAN_BLOCK_WINDOW, WC.STRADDLE[(520, 264)], (0, 0, 8, 8), (512, 256, 8, 8), (0, 128, 520, 8)])
def test_planes_outside_the_windows_blocks_keep_the_previous_image(dec, oracle_built, win, path):
    w, h, kind = 520, 264, "mixed"
    ref_a, key_a = _refs(w, h, kind)
    ref_b, key_b = _refs(w, h, kind, second=True)
    dec.begin(w, h)
    _decode(dec, ref_a, key_a, path)
    assert np.array_equal(dec.planes(), ref_a.planes)
    dec.begin(w, h)
    dec.set_window(*win)
    _decode(dec, ref_b, key_b, path)
    got = WC.tiles_of(dec.planes(), w, h)
    a, b = WC.tiles_of(ref_a.planes, w, h), WC.tiles_of(ref_b.planes, w, h)
    x0, y0, ww, wh = win
    inside = np.s_[:, y0 // 8:(y0 + wh) // 8, x0 // 8:(x0 + ww) // 8]
    assert np.array_equal(got[inside], b[inside])
    outside = WC.outside_rounded(w, h, win)
    assert outside.any()
    assert np.array_equal(got[:, outside], a[:, outside]), "a tile outside the window's 64-blocks was written"
    assert (a[:, outside] != b[:, outside]).any()                            # ... and the two images differ there, so a write would show
    assert np.array_equal(dec.tile4x4(), ref_b.tile4)
    assert np.array_equal(dec.image_window_device().cpu().numpy(), ref_b.crop(win))


# ---- encoder streams at 2048 x 2048 --------------------------------------------------------------------------------------------------------
def test_encoder_streams_2048_random_windows(dec, dec2):
    torch = _torch()
    from yaik_amd.encoder import HipTileEncoder
    from yaik_amd.synth import synth_planes
    n = 2048
    enc = HipTileEncoder(0)
    try:
        enc.set_image(synth_planes(n, n_planes=3))
        enc.encode(3, False, False)
        calls = dec2.encoder_streams(enc)
        dec2.begin(n, n)
        dec2.decode_streams(calls)
        whole = dec2.image_device()
        want4 = dec2.tile4x4()
        rng = np.random.default_rng(2048)
        wins = [(0, 0, n, n)]
        while len(wins) < 9:
            ww, wh = (int(rng.integers(1, 65)) * 8 for _ in range(2))
            x0, y0 = int(rng.integers(0, (n - ww) // 8 + 1)) * 8, int(rng.integers(0, (n - wh) // 8 + 1)) * 8
            wins.append((x0, y0, ww, wh))
        for k, win in enumerate(wins):
            x0, y0, ww, wh = win
            dec.begin(n, n)
            dec.set_window(*win)
            dec.decode_streams(calls, per_pass=bool(k & 1))
            got = dec.image_window_device()
            assert torch.equal(got, whole[y0:y0 + wh, x0:x0 + ww]), win
            assert np.array_equal(dec.tile4x4(), want4), win
    finally:
        dec.synchronize(); dec2.synchronize()
        enc.close()


# ---- files ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files():
    from yaik_amd import files as F
    F.set_device_palette(False)
    yield F
    F.set_device_palette(False)


@pytest.fixture(scope="module")
def file_streams(files):
    """(rgb, rgba): streams of a 136 x 264 "mixed" frame from encode_file_device, without and with an 'ALPM' chunk"""
    torch = _torch()
    from tests.images import edge_image
    planes = edge_image(136, 264, "mixed", 4)
    hwc = torch.from_numpy(np.ascontiguousarray(planes.transpose(1, 2, 0)).astype(np.uint8)).cuda()
    rgb = files.encode_file_device(hwc[..., :3].contiguous())
    rgba = files.encode_file_device(hwc, emit_alpha=True)
    assert not files.has_alpha_chunk(rgb) and files.has_alpha_chunk(rgba)
    return rgb, rgba


@pytest.mark.parametrize("palette", [False, True])
def test_file_windows_equal_the_crop_of_the_whole_file_decode(files, file_streams, palette):
    torch = _torch()
    files.set_device_palette(palette)
    try:
        for stream, c in zip(file_streams, (3, 4)):
            whole = files.decode_file_device(stream)
            assert tuple(whole.shape) == (264, 136, c)
            for win in WC.windows(136, 264):
                x0, y0, ww, wh = win
                got = files.decode_file_window_device(stream, win)
                assert tuple(got.shape) == (wh, ww, c) and torch.equal(got, whole[y0:y0 + wh, x0:x0 + ww]), (c, win)
            assert torch.equal(files.decode_file_device(stream), whole)         # the slot's handle goes back to whole images
    finally:
        files.set_device_palette(False)


def test_file_window_outside_the_image_is_refused(files, file_streams):
    from yaik_amd.files import ERROR_NAMES, YaikFileError
    for win in ((136, 0, 8, 8), (0, 264, 8, 8), (8, 0, 136, 8), (0, 8, 8, 264)):
        with pytest.raises(YaikFileError) as e:
            files.decode_file_window_device(file_streams[0], win)
        assert ERROR_NAMES[e.value.code] == "YAIK_DECIMG_INVALIDCTX"
    assert files.decode_file_window_device(file_streams[0], (0, 0, 8, 8)).shape == (8, 8, 3)      # the slot was released each time


def _gtil_chunks(stream):
    out, p = [], 12
    while p + 8 <= len(stream):
        tag, ln = struct.unpack_from("<II", stream, p)
        if tag == 0xDEADBEEF:
            break
        if tag == TAG_GTIL:
            out.append(p + 8)
        p += 8 + ln
    return out


def test_file_with_a_plane_subset_chunk_still_gives_the_exact_crop(files, file_streams):
    """The 4x4 'GTIL' chunk of a stream re-labelled as an R+G chunk (HeaderGradientTile::plane = 3): the masks are split, the plane-subset
    kernels and the per-plane 1-D decode run, all of which ignore the window and write the whole image.  What the file then decodes to is
    whatever the whole-file decode makes of it; the window is its crop."""
    torch = _torch()
    stream = bytearray(file_streams[0])
    bodies = [b for b in _gtil_chunks(stream) if stream[b + 26] & 7 == 2 and (stream[b + 26] >> 3) & 7 == 2]
    assert len(bodies) == 1 and stream[bodies[0] + 27] == 7
    stream[bodies[0] + 27] = 3
    stream = bytes(stream)
    whole = files.decode_file_device(stream)
    assert not torch.equal(whole, files.decode_file_device(file_streams[0]))   # the chunk was really read another way
    for win in WC.windows(136, 264):
        x0, y0, ww, wh = win
        assert torch.equal(files.decode_file_window_device(stream, win), whole[y0:y0 + wh, x0:x0 + ww]), win


def test_plane_subset_chunks_under_a_window_match_the_oracle(dec, oracle_built):
    from oracle.pyoracle import PASSES, OracleDecoder, OracleEncoder, detile, palette_remap
    from tests.blobs import PP_MASKS
    from tests.images import edge_image
    w, h = 200, 72
    planes = edge_image(w, h, "planemix", 3)
    ora, od = OracleEncoder(planes), OracleDecoder(w, h)
    steps = []
    for sx, sy in PASSES:
        cnt, bm, rgb = ora.fitting_quad_smooth(sx, sy)
        if cnt:
            dq = palette_remap(rgb, 250)
            od.gradient(sx, sy, bm, dq); steps.append(("g", sx, sy, bm, dq))
    od.split_masks()
    for m in PP_MASKS:
        cnt, bm, rgb = ora.fitting_quad_smooth(2, 2, plane_bit=m)
        if cnt:
            dq = palette_remap(rgb, 250)
            od.gradient_planes(m, bm, dq, consistent_marks=True); steps.append(("p", m, bm, dq))
    assert any(s[0] == "p" for s in steps)
    for p in range(3):
        ora.dynamic_tile_compressor(p)
    pix, typ = ora.streams_1d()
    od.decode_1d(typ, pix)
    want = np.stack([detile(od.planes()[c], w, h) for c in range(3)], axis=-1)
    for win in ((0, 0, w, h), (56, 8, 16, 56), (192, 64, 8, 8), (0, 32, 200, 8)):
        dec.begin(w, h)
        dec.set_window(*win)
        for s in steps:
            if s[0] == "g":
                dec.decompress_gradient(*s[1:])
            else:
                dec.decompress_gradient_planes(s[1], s[2], s[3], consistent_marks=True)
        dec.decompress_1d(typ, pix)
        x0, y0, ww, wh = win
        assert np.array_equal(dec.image_window_device().cpu().numpy(), want[y0:y0 + wh, x0:x0 + ww]), win
        assert np.array_equal(dec.tile4x4(all_planes=True), od.tile4x4(all_planes=True))


def test_3dtl_chunk_under_a_window_matches_the_reference_fixture(dec, oracle_built):
    import os
    from oracle.pyoracle import PASSES, OracleEncoder, detile, palette_decompress, palette_remap
    from tests.golden.make_golden import LUT3D
    name = "lut_lutmix128_rgb"
    ref = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))
    planes, _ = LUT3D[name]()
    _, h, w = planes.shape
    ora = OracleEncoder(planes)
    grads = []
    for sx, sy in PASSES:
        cnt, bm, rgb = ora.fitting_quad_smooth(sx, sy)
        if cnt:
            grads.append((sx, sy, bm, palette_decompress(ora.palette_compress(rgb), rgb.size, 250)))
    zin = [ref[f"lut_zin_{k}"] for k in range(len([k for k in ref if k.startswith("lut_zin_")]))]
    counts = np.frombuffer(ref["lut_counts"].tobytes(), np.int32).reshape(6, 6)[-1]
    it = iter(zin[6:])
    tiles = next(it).view(np.uint16) if counts[0] else np.zeros(0, np.uint16)
    colors = palette_remap(next(it), 250) if counts[1] else np.zeros(0, np.uint8)
    idx = [next(it) if counts[2 + f] else np.zeros(0, np.uint8) for f in range(4)]
    full = ref["dec_planes_full"].reshape(3, -1)
    want = np.stack([detile(full[c], w, h) for c in range(3)], axis=-1)
    for win in ((0, 0, w, h), (56, 56, 16, 16), (w - 8, h - 8, 8, 8), (0, 64, w, 8)):
        dec.begin(w, h)
        dec.set_window(*win)
        for g in grads:
            dec.decompress_gradient(*g)
        dec.assign_lut(ref["lut_file"])
        dec.decompress_lut3d(zin[:6], tiles, colors, idx)
        dec.decompress_1d(ref["d1_type"], ref["d1_pix"])
        x0, y0, ww, wh = win
        assert np.array_equal(dec.image_window_device().cpu().numpy(), want[y0:y0 + wh, x0:x0 + ww]), win


# ---- state and arguments -------------------------------------------------------------------------------------------------------------------
def _rc(fn, *args):
    return int(fn(*args))


def test_set_window_state_and_argument_refusals(dec, oracle_built):
    from yaik_amd._lib import YaikError, lib
    from yaik_amd.decoder import HipTileDecoder
    L = lib()
    w, h, kind = 136, 264, "mixed"
    ref, key = _refs(w, h, kind)
    fresh = HipTileDecoder(0)
    try:
        assert _rc(L.yk_decode_set_window, fresh._h, 0, 0, 8, 8) == YK_ERR_STATE        # before any begin
        assert b"yk_decode_begin" in L.yk_last_error(fresh._h)
        fresh.begin_batch(w, h, 2)
        assert _rc(L.yk_decode_set_window, fresh._h, 0, 0, 8, 8) == YK_ERR_STATE        # a batch
        fresh.begin_batch(w, h, 1)
        assert _rc(L.yk_decode_set_window, fresh._h, 0, 0, 8, 8) == YK_ERR_STATE        # ... of one frame as well
        assert b"batch" in L.yk_last_error(fresh._h)
        with pytest.raises(YaikError, match="batch"):
            fresh.set_window(0, 0, 8, 8)
        assert fresh.window is None
    finally:
        fresh.close()
    dec.begin(w, h)
    for bad in ((4, 0, 8, 8), (0, 4, 8, 8), (0, 0, 12, 8), (0, 0, 8, 12), (0, 0, 0, 8), (0, 0, 8, 0), (-8, 0, 8, 8), (0, -8, 8, 8), (136, 0, 8, 8),
                (0, 264, 8, 8), (8, 0, 136, 8), (0, 8, 8, 264), (0, 0, 144, 8), (0, 0, 8, 272), (0, 0, -8, -8), (2 ** 31 - 8, 0, 16, 8)):
        assert _rc(L.yk_decode_set_window, dec._h, *bad) == YK_ERR_BAD_ARG, bad
    assert b"window" in L.yk_last_error(dec._h)
    dec.set_window(8, 16, 64, 32)
    dec.set_window(0, 0, 0, 0)                                               # ww == wh == 0 clears
    assert dec.window is None
    dec.set_window(8, 16, 64, 32)
    dec.begin(w, h)                                                          # begin clears
    assert dec.window is None
    _decode(dec, ref, key, "per_pass")
    assert np.array_equal(dec.image_device().cpu().numpy(), ref.rgb)         # whole-image calls work: no window survived the begin
    # after a chunk: too late, for a window and for clearing one
    for args in ((0, 0, 8, 8), (0, 0, 0, 0)):
        assert _rc(L.yk_decode_set_window, dec._h, *args) == YK_ERR_STATE
    assert b"chunk" in L.yk_last_error(dec._h)
    for first in ("gradient", "1d", "split"):
        dec.begin(w, h)
        if first == "gradient":
            _decode(dec, ref, key, "all_pass", gradients_only=True)
        elif first == "1d":
            dec.decompress_1d(ref.typ, ref.pix)
        else:
            assert L.yk_decode_split_masks(dec._h) == 0
        assert _rc(L.yk_decode_set_window, dec._h, 0, 0, 8, 8) == YK_ERR_STATE, first
    # an 'ALPM' plane is whole-image and no chunk of the planes: the window may follow it
    dec.begin(w, h)
    _alpha_plane(dec, w, h, 3)
    dec.set_window(0, 0, 8, 8)


def test_whole_image_calls_refuse_under_a_window(dec, oracle_built):
    torch = _torch()
    from yaik_amd._lib import YaikError, lib
    L = lib()
    w, h, kind = 136, 264, "mixed"
    ref, key = _refs(w, h, kind)
    win = (56, 56, 24, 16)
    dec.begin(w, h)
    dec.set_window(*win)
    alpha = _alpha_plane(dec, w, h, 5)
    _decode(dec, ref, key, "all_pass")
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    ok = dec.image_window_device()
    for call in (lambda: dec.image(), lambda: dec.image(alpha=alpha), lambda: dec.image(alpha=alpha, reference_rgba=True),
                 lambda: dec.image_into(np.zeros((h, w * 3), np.uint8)), lambda: dec.image_device(), lambda: dec.image_device(channels=3),
                 lambda: dec.compare_device(src), lambda: dec.compare_planes(torch.zeros((3, h, w), dtype=torch.int32, device="cuda"))):
        with pytest.raises(YaikError, match="window") as e:
            call()
        assert f"error {YK_ERR_STATE}" in str(e.value)
    q = (C.c_uint8 * 4096)()
    assert _rc(L.yk_decode_compare_batch_device, dec._h, src.data_ptr(), w * 3, 0, 0, 3, 3, q, None) == YK_ERR_STATE
    assert b"window" in L.yk_last_error(dec._h)
    # the refusals left everything as it was; planes, marks and the alpha plane stay readable
    assert torch.equal(dec.image_window_device(), ok)
    assert np.array_equal(ok.cpu().numpy()[..., :3], ref.crop(win))
    assert np.array_equal(dec.tile4x4(), ref.tile4) and np.array_equal(dec.alpha_plane(), alpha)
    assert dec.planes().shape == (3, (w // 8) * (h // 8) * 64)
    # bad layouts for the window are refused by the library too
    out = torch.empty((win[3], win[2], 3), dtype=torch.uint8, device="cuda")
    assert _rc(L.yk_decode_output_window_device, dec._h, out.data_ptr(), win[2] * 3 - 1, 0, 3, 0) == YK_ERR_BAD_ARG
    assert _rc(L.yk_decode_output_window_device, dec._h, None, win[2] * 3, 0, 3, 0) == YK_ERR_BAD_ARG
    assert _rc(L.yk_decode_output_window_device, dec._h, out.data_ptr(), win[2] * 3, 0, 5, 0) == YK_ERR_BAD_ARG
    assert _rc(L.yk_decode_output_window_device, dec._h, out.data_ptr(), win[2], win[2] * win[3] - 1, 3, 0) == YK_ERR_BAD_ARG


def test_without_a_window_the_output_call_is_the_whole_image_call(dec, oracle_built):
    w, h, kind = 136, 264, "mixed"
    ref, key = _refs(w, h, kind)
    dec.begin(w, h)
    _decode(dec, ref, key, "all_pass")
    assert np.array_equal(dec.image_window_device().cpu().numpy(), ref.rgb)
    assert np.array_equal(dec.image_window_device(planar=True, channels=4, alpha=9).cpu().numpy()[:3], ref.rgb.transpose(2, 0, 1))


def test_one_detile_interval_per_output_call(dec, oracle_built):
    w, h, kind = 136, 264, "mixed"
    ref, key = _refs(w, h, kind)
    stage = YK_STAGE_DEC_DETILE
    dec.begin(w, h)
    dec.set_window(64, 0, 8, 264)
    _decode(dec, ref, key, "all_pass")
    dec.synchronize()
    dec.stage_ms(stage)                                                      # fold what earlier tests left
    for n in (1, 3):
        for _ in range(n):
            dec.image_window_device()
        dec.synchronize()
        ms, calls = dec.stage_ms(stage)
        assert calls == n and ms > 0


@pytest.mark.parametrize("path", ["per_pass", "all_pass"])
def test_handle_reused_whole_window_whole(dec, oracle_built, path):
    w, h, kind = 520, 264, "mixed"
    ref_a, key_a = _refs(w, h, kind)
    ref_b, key_b = _refs(w, h, kind, second=True)
    for ref, key, win in ((ref_a, key_a, None), (ref_b, key_b, WC.SCAN_BLOCK_WINDOW), (ref_a, key_a, None), (ref_b, key_b, (0, 0, 8, 8)), (ref_b, key_b, None)):
        dec.begin(w, h)
        if win is not None:
            dec.set_window(*win)
        _decode(dec, ref, key, path)
        if win is None:
            assert np.array_equal(dec.image_device().cpu().numpy(), ref.rgb)
            assert np.array_equal(dec.planes(), ref.planes)
        else:
            assert np.array_equal(dec.image_window_device().cpu().numpy(), ref.crop(win))
        assert np.array_equal(dec.tile4x4(), ref.tile4)


def test_settle_under_a_window_zeroes_the_windows_unmarked_cells(dec, oracle_built):
    """gradient passes only, then an output call: what no chunk wrote reads as zero inside the window, like the whole-image flow"""
    w, h, kind = 520, 264, "mixed"
    ref_a, key_a = _refs(w, h, kind)
    ref_b, key_b = _refs(w, h, kind, second=True)
    dec.begin(w, h)
    _decode(dec, ref_a, key_a, "all_pass")                                   # the planes hold image A
    dec.begin(w, h)
    _decode(dec, ref_b, key_b, "all_pass", gradients_only=True)
    whole = dec.image_device().cpu().numpy()                                 # B's gradient tiles, zeros elsewhere
    dec.begin(w, h)
    _decode(dec, ref_a, key_a, "all_pass")
    win = WC.SCAN_BLOCK_WINDOW
    dec.begin(w, h)
    dec.set_window(*win)
    _decode(dec, ref_b, key_b, "all_pass", gradients_only=True)
    x0, y0, ww, wh = win
    assert np.array_equal(dec.image_window_device().cpu().numpy(), whole[y0:y0 + wh, x0:x0 + ww])
