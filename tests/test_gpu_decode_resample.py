"""Per-frame rectangles resampled to one output size on the GPU (yk_decode_set_batch_rects, yk_decode_output_resampled_batch_device,
yk_decode_output_resampled_device, YAIK_DecodeImagesResampledToDevice) against tests/resample_ref.py on the oracle's whole decode.  The
contract is fully defined in integers, so every comparison is exact: rectangle sets whose sizes differ per frame in every element type, identity and
2x against the existing calls, every layout into sentinel-filled padded buffers, the planes outside each frame's cover, back-to-back batches, the
single-image call, every refusal, `.yaik` files, and the existing calls after the new ones."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_window_cases as BW
from tests import norm_ref as NR
from tests import resample_ref as RR
from tests import window_cases as WC
from tests.test_gpu_decode_batch_window import _alpha_entries, _decode_batch
from tests.test_gpu_decode_window import _decode, _refs

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_STAGE_DEC_DETILE = -2, -4, 5
SCALE, BIAS = NR.parameter_sets()["B"]
ELEMS = (None,) + NR.DTYPES


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _norm(dtype):
    return {} if dtype is None else dict(dtype=dtype, scale=SCALE, bias=BIAS)


def _bits(t, dtype):
    return t.cpu().numpy() if dtype is None else NR.bits(t)


def _rgba(rgb, alpha):
    a = np.full(rgb.shape[:-1], alpha, np.uint8) if np.isscalar(alpha) else alpha
    return np.concatenate([rgb, a[..., None]], axis=-1)


def _batch_alpha(d, n):
    out = []
    for f in range(n):
        d.select_frame(f)
        out.append(d.alpha_plane())
    d.select_frame(0)
    return out


def _begin_rects(d, refs, rects, alpha_seed=None, sync=True):
    """begin_batch + set_batch_rects + (alpha planes) + the chunks of every frame; returns the RGBA whole decode of every frame"""
    w, h, n = refs[0].w, refs[0].h, len(refs)
    d.begin_batch(w, h, n)
    if rects is not None:
        d.set_batch_rects(rects)
    if alpha_seed is not None:
        d.decompress_alpha_batch(_alpha_entries(w, h, n, seed=alpha_seed), 255, sync=False)
    _decode_batch(d, refs, sync=sync)
    alpha = _batch_alpha(d, n) if alpha_seed is not None else [255] * n
    return [_rgba(r.rgb, a) for r, a in zip(refs, alpha)]


# ---- 1: rectangle sets whose sizes differ per frame, every element type, mixed mirror flags ---------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_a", "mixed_b"])
@pytest.mark.parametrize("w,h,kind,n", BW.BATCHES, ids=_ids)
def test_every_rectangle_equals_the_reference(dec, oracle_built, w, h, kind, n, name):
    refs = BW.batch_references(w, h, kind, n)
    rects = RR.RECT_SETS[(w, h)][name]
    flags = RR.FLAGS[:n]
    wholes = _begin_rects(dec, refs, np.asarray(rects, dtype=np.int64), alpha_seed=w + h + n)
    assert np.array_equal(dec.batch_rects, np.asarray(rects, np.int32)) and dec.batch_windows is None
    for size in RR.SIZES:
        for dtype in ELEMS:
            got = dec.image_resampled_batch_device(size, mirror=flags, channels=4, alpha_from_planes=True, **_norm(dtype))
            assert tuple(got.shape) == (n, size[1], size[0], 4)
            want = RR.batch_ref(wholes, rects, size, dtype, SCALE, BIAS, flags)
            assert np.array_equal(_bits(got, dtype), want), (size, dtype)
        got = dec.image_resampled_batch_device(size, channels=3)                                      # no flags, three channels, uint8
        assert np.array_equal(got.cpu().numpy(), RR.batch_ref([wh[..., :3] for wh in wholes], rects, size))


def test_whole_frames_without_rectangles(dec, oracle_built):
    w, h, kind, n = 136, 264, "mixed", 3
    refs = BW.batch_references(w, h, kind, n)
    wholes = _begin_rects(dec, refs, None)
    whole = [(0, 0, w, h)] * n
    for size in ((13, 11), (136, 264), (300, 7)):
        got = dec.image_resampled_batch_device(size, mirror=[0, 1, 0])
        assert np.array_equal(got.cpu().numpy(), RR.batch_ref([v[..., :3] for v in wholes], whole, size, flags=[0, 1, 0])), size


# ---- 2: identity sizes and 2x against the existing calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,n", BW.BATCHES[:2], ids=_ids)
def test_identity_equals_the_pixel_windows_and_two_times_the_box_mean(dec, oracle_built, w, h, kind, n):
    torch = _torch()
    refs = BW.batch_references(w, h, kind, n)
    size = (13, 11)
    origins = [(3, 5), (w - 13, h - 11), (61, 59), (70, 9)][:n]
    flags = RR.FLAGS[:n]
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, *size, px=True)
    _decode_batch(dec, refs)
    win_u8 = dec.image_batch_windows_device().clone()
    win_nrm = {dt: dec.image_norm_batch_device(dt, scale=SCALE, bias=BIAS, mirror=flags, planar=True).clone() for dt in NR.DTYPES}
    _begin_rects(dec, refs, [o + size for o in origins])
    assert torch.equal(dec.image_resampled_batch_device(size), win_u8)
    for dt in NR.DTYPES:
        got = dec.image_resampled_batch_device(size, mirror=flags, planar=True, **_norm(dt))
        assert np.array_equal(NR.bits(got), NR.bits(win_nrm[dt])), dt
    # 2x on aligned rectangles: the level-1 box mean, cropped
    rects = [(64, 32, 64, 128), (0, 0, 16, 16), (w - 72, h - 40, 48, 32), (8, 136, 128, 64)][:n]
    dec.begin_batch(w, h, n)
    _decode_batch(dec, refs)
    half = dec.image_scaled_batch_device(1).cpu().numpy()
    for f, (x0, y0, sw, sh) in enumerate(rects):                                                       # sizes differ, so one rectangle for all frames per call
        _begin_rects(dec, refs, [rects[f]] * n)
        got = dec.image_resampled_batch_device((sw // 2, sh // 2)).cpu().numpy()
        assert np.array_equal(got[f], half[f, y0 // 2:(y0 + sh) // 2, x0 // 2:(x0 + sw) // 2]), f


# ---- 3: layouts; every byte outside the pixels keeps the sentinel ------------------------------------------------------------------------------
def _padded(dtype, shape, planar, batch):
    """a sentinel-filled byte buffer and a view of it (uint8 for dtype None) of `shape` at an odd element offset with row, plane and frame padding;
    returns (bytes [n, es], view, mask [n] of the elements the view covers)"""
    torch = _torch()
    tdt, es = (torch.uint8, 1) if dtype is None else (getattr(torch, dtype), NR.ELEM_BYTES[dtype])
    if planar:
        c, hh, ww = shape[-3:]
        row = ww + 11
        plane = row * hh + 13
        frame, strides, off = plane * c + 29, (plane, row, 1), 3
    else:
        hh, ww, c = shape[-3:]
        row = ww * c + 11
        frame, strides, off = row * hh + 29, (row, c, 1), 5
    n = off + frame * (shape[0] if batch else 1) + 64
    if batch:
        strides = (frame,) + strides
    raw = torch.full((n * es,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(raw.view(tdt), shape, strides, off)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.as_strided(mask, shape, strides, off).fill_(True)
    return raw.view(n, es), view, mask


LAYOUTS = [(3, None, False), (4, 77, False), (4, None, False), (3, None, True), (4, None, True), (4, 77, True)]   # channels, alpha (None: the planes), planar


@pytest.mark.parametrize("dtype", ELEMS, ids=str)
def test_layouts_write_the_pixels_and_nothing_else(dec, oracle_built, dtype):
    w, h, kind, n = 136, 264, "mixed", 3
    refs = BW.batch_references(w, h, kind, n)
    rects = RR.RECT_SETS[(w, h)]["mixed_a"]
    flags = RR.FLAGS[:n]
    w0, h0 = refs[0].w, refs[0].h
    dec.begin_batch(w0, h0, n)
    dec.set_batch_rects(rects)
    # a plane holding all 256 values: mode 6 payloads over the whole frame
    rng = np.random.default_rng(7)
    entries = [(6, (0, 0, w, h), np.concatenate([np.arange(256, dtype=np.uint8), rng.integers(0, 256, w * h - 256).astype(np.uint8)])) for _ in range(n)]
    dec.decompress_alpha_batch(entries, 255, sync=False)
    _decode_batch(dec, refs)
    alpha = _batch_alpha(dec, n)
    assert all(len(np.unique(a)) == 256 for a in alpha)
    for size in ((13, 11), (7, 3)):
        for channels, a_arg, planar in LAYOUTS:
            wholes = [r.rgb if channels == 3 else _rgba(r.rgb, a if a_arg is None else a_arg) for r, a in zip(refs, alpha)]
            want = RR.batch_ref(wholes, rects, size, dtype, SCALE, BIAS, flags)
            want = np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if planar else want
            raw, view, mask = _padded(dtype, want.shape, planar, True)
            got = dec.image_resampled_batch_device(size, mirror=flags, out=view, channels=channels, alpha=255 if a_arg is None else a_arg, planar=planar,
                                                   alpha_from_planes=channels == 4 and a_arg is None, **_norm(dtype))
            assert got is view and np.array_equal(_bits(view, dtype), want), (size, channels, a_arg, planar)
            assert bool((raw[~mask] == SENTINEL).all()), (size, channels, a_arg, planar, "a byte outside the pixels changed")


# ---- 4: the planes outside each frame's cover rounded out to 64 are not written ------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,n", BW.BATCHES[:2], ids=_ids)
def test_planes_outside_each_frames_blocks_keep_the_previous_batch(dec, oracle_built, w, h, kind, n):
    refs_a, refs_b = BW.batch_references(w, h, kind, n), BW.batch_references(w, h, kind, n, second=True)
    for name, rects in RR.rect_sets(w, h):
        dec.begin_batch(w, h, n)
        _decode_batch(dec, refs_a)
        dec.begin_batch(w, h, n)
        dec.set_batch_rects(rects)
        _decode_batch(dec, refs_b)
        checked = 0
        for f, rect in enumerate(rects):
            dec.select_frame(f)
            got = WC.tiles_of(dec.planes(), w, h)
            a, b = WC.tiles_of(refs_a[f].planes, w, h), WC.tiles_of(refs_b[f].planes, w, h)
            cx0, cy0, cx1, cy1 = RR.cover(rect)
            inside = np.s_[:, cy0 // 8:cy1 // 8, cx0 // 8:cx1 // 8]
            assert np.array_equal(got[inside], b[inside]), (name, f)
            assert np.array_equal(dec.tile4x4(), refs_b[f].tile4), (name, f)
            outside = WC.outside_rounded(w, h, (cx0, cy0, cx1 - cx0, cy1 - cy0))
            if not outside.any():                                                                      # the whole frame
                continue
            checked += 1
            assert np.array_equal(got[:, outside], a[:, outside]), (name, f, "a tile outside the cover's 64-blocks was written")
            assert (a[:, outside] != b[:, outside]).any()                                              # the two batches differ there, so a write would show
        assert checked >= n - 1
        dec.select_frame(0)
        assert np.array_equal(dec.image_resampled_batch_device((13, 11)).cpu().numpy(), RR.batch_ref([r.rgb for r in refs_b], rects, (13, 11))), name


def test_settle_zeroes_the_unmarked_cells_of_each_frames_cover(dec, oracle_built):
    """gradient chunks only, then an output: what no chunk wrote reads as zero inside each rectangle, as in the whole-batch flow"""
    w, h, kind, n = 520, 264, "mixed", 4
    refs_a, refs_b = BW.batch_references(w, h, kind, n), BW.batch_references(w, h, kind, n, second=True)
    rects = RR.RECT_SETS[(w, h)]["mixed_b"]
    dec.begin_batch(w, h, n)
    _decode_batch(dec, refs_b, gradients_only=True)
    whole = dec.image_batch_device().cpu().numpy()                           # B's gradient tiles, zeros elsewhere
    dec.begin_batch(w, h, n)
    _decode_batch(dec, refs_a)
    dec.begin_batch(w, h, n)
    dec.set_batch_rects(rects)
    _decode_batch(dec, refs_b, gradients_only=True)
    got = dec.image_resampled_batch_device((56, 40)).cpu().numpy()
    assert np.array_equal(got, RR.batch_ref(list(whole), rects, (56, 40)))
    assert (whole == 0).any()


# ---- 5: tables of queued calls; rectangles and windows replace each other ----------------------------------------------------------------------
def test_two_batches_back_to_back_read_their_own_tables(dec, oracle_built):
    w, h, kind, n = 136, 264, "mixed", 3
    refs_a, refs_b = BW.batch_references(w, h, kind, n), BW.batch_references(w, h, kind, n, second=True)
    r_a, r_b = RR.RECT_SETS[(w, h)]["mixed_a"], RR.RECT_SETS[(w, h)]["mixed_b"]
    f_a, f_b = [True, False, True], [False, True, True]
    dec.begin_batch(w, h, n)
    dec.set_batch_rects(r_a)
    _decode_batch(dec, refs_a, sync=False)
    out_a = dec.image_resampled_batch_device((13, 11), mirror=f_a)            # queued; the next batch's tables are written behind it
    dec.begin_batch(w, h, n)
    dec.set_batch_rects(r_b)
    _decode_batch(dec, refs_b, sync=False)
    out_b = dec.image_resampled_batch_device((13, 11), mirror=f_b)
    out_c = dec.image_resampled_batch_device((56, 40), mirror=f_a, dtype="float16", scale=SCALE, bias=BIAS)     # the same batch, other size and flags, no fence
    out_d = dec.image_resampled_batch_device((13, 11), mirror=f_a)
    dec.synchronize()
    rgb = lambda refs: [r.rgb for r in refs]
    assert np.array_equal(out_a.cpu().numpy(), RR.batch_ref(rgb(refs_a), r_a, (13, 11), flags=f_a))
    assert np.array_equal(out_b.cpu().numpy(), RR.batch_ref(rgb(refs_b), r_b, (13, 11), flags=f_b))
    assert np.array_equal(NR.bits(out_c), RR.batch_ref(rgb(refs_b), r_b, (56, 40), "float16", SCALE, BIAS, f_a))
    assert np.array_equal(out_d.cpu().numpy(), RR.batch_ref(rgb(refs_b), r_b, (13, 11), flags=f_a))
    assert not np.array_equal(out_b.cpu().numpy(), out_d.cpu().numpy())


def test_rectangles_and_windows_replace_each_other(dec, oracle_built):
    w, h, kind, n = 136, 264, "mixed", 3
    refs = BW.batch_references(w, h, kind, n)
    rects = RR.RECT_SETS[(w, h)]["mixed_b"]
    origins, size = [(3, 5), (123, 253), (61, 59)], (13, 11)
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, *size, px=True)
    dec.set_batch_rects(rects)                                                # rectangles after windows
    assert dec.batch_windows is None and dec.batch_rects is not None
    _decode_batch(dec, refs)
    with pytest.raises(Exception, match="rectangles"):
        dec.image_batch_windows_device()
    assert np.array_equal(dec.image_resampled_batch_device((7, 3)).cpu().numpy(), RR.batch_ref([r.rgb for r in refs], rects, (7, 3)))
    dec.begin_batch(w, h, n)
    dec.set_batch_rects(rects)
    dec.set_batch_windows(origins, *size, px=True)                            # windows after rectangles
    assert dec.batch_rects is None and dec.batch_windows is not None
    _decode_batch(dec, refs)
    assert np.array_equal(dec.image_batch_windows_device().cpu().numpy(), BW.crops(refs, size, origins))
    with pytest.raises(Exception, match="windows"):
        dec.image_resampled_batch_device((7, 3))
    dec.begin_batch(w, h, n)
    dec.set_batch_rects(rects)
    dec.set_batch_rects(None)                                                 # cleared: whole frames again
    _decode_batch(dec, refs)
    assert np.array_equal(dec.image_batch_device().cpu().numpy(), np.stack([r.rgb for r in refs]))


# ---- 6: the single-image call ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ELEMS, ids=str)
def test_single_image_call(dec, oracle_built, dtype):
    w, h, kind = 136, 264, "mixed"
    ref, key = _refs(w, h, kind)
    cases = [(None, False, [None, (3, 5, 101, 97), (67, 131, 1, 1), (0, 0, w, h)]),
             ((8, 8, 120, 240), False, [None, (8, 8, 120, 240), (9, 11, 101, 97), (127, 247, 1, 1)]),
             ((3, 5, 101, 97), True, [None, (3, 5, 101, 97), (4, 6, 3, 2), (103, 101, 1, 1)])]
    for win, px, rects in cases:
        dec.begin(w, h)
        if win is not None:
            dec.set_window(*win, px=px)
        _decode(dec, ref, key, "all_pass")
        for rect in rects:
            full = rect if rect is not None else win if win is not None else (0, 0, w, h)
            for size, mirror in (((13, 11), False), ((7, 3), True), ((1, 1), True)):
                got = dec.image_resampled_device(size, rect=rect, mirror=mirror, channels=4, alpha=9, **_norm(dtype))
                want = RR.resample_ref(_rgba(ref.rgb, 9), full, size, dtype, SCALE, BIAS, mirror)
                assert np.array_equal(_bits(got, dtype), want), (win, rect, size)
        if win is not None:                                                   # a rectangle outside the window: the library refuses, nothing is written
            torch = _torch()
            from yaik_amd._lib import lib
            out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
            x0, y0, ww, wh = win
            for bad in ((x0 - 1, y0, 4, 4), (x0, y0 - 1, 4, 4), (x0 + ww - 3, y0, 4, 4), (x0, y0 + wh - 3, 4, 4)):
                r = (C.c_int * 4)(*bad)
                assert int(lib().yk_decode_output_resampled_device(dec._h, r, None, 0, out.data_ptr(), 8, 8, 24, 0, 3, 255)) == YK_ERR_BAD_ARG, bad
                assert b"yk_decode_output_resampled_device" in lib().yk_last_error(dec._h) and b"window" in lib().yk_last_error(dec._h)
            assert bool((out == SENTINEL).all())
    # the selected frame of a batch that has neither rectangles nor windows
    n = 3
    refs = BW.batch_references(w, h, kind, n)
    dec.begin_batch(w, h, n)
    _decode_batch(dec, refs)
    dec.select_frame(2)
    got = dec.image_resampled_device((13, 11), rect=(3, 5, 101, 97), mirror=True, **_norm(dtype))
    assert np.array_equal(_bits(got, dtype), RR.resample_ref(refs[2].rgb, (3, 5, 101, 97), (13, 11), dtype, SCALE, BIAS, True))
    dec.select_frame(0)


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_first_and_leave_the_handle_usable(dec, oracle_built):
    torch = _torch()
    from yaik_amd._lib import lib
    from yaik_amd.decoder import HipTileDecoder
    from yaik_amd.encoder import NormC
    L = lib()
    w, h, kind, n = 136, 264, "mixed", 3
    f4 = lambda *v: (C.c_float * 4)(*v)
    good, f32 = NormC(1, f4(1, 1, 1, 1), f4(0, 0, 0, 0)), NormC(3, f4(1, 1, 1, 1), f4(0, 0, 0, 0))
    out = torch.full((8192,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = out.data_ptr()
    assert p % 4 == 0
    setr, single, batch = L.yk_decode_set_batch_rects, L.yk_decode_output_resampled_device, L.yk_decode_output_resampled_batch_device
    ow, oh = 13, 11
    row = ow * 3
    tab = lambda rects: (C.c_int * (4 * len(rects)))(*[v for r in rects for v in r])
    good_rects = RR.RECT_SETS[(w, h)]["mixed_a"]
    fresh = HipTileDecoder(0)
    try:                                                                      # before any begin
        assert int(setr(fresh._h, tab(good_rects))) == YK_ERR_STATE and b"yk_decode_set_batch_rects" in L.yk_last_error(fresh._h)
        assert int(single(fresh._h, None, None, 0, p, ow, oh, row, 0, 3, 255)) == YK_ERR_STATE and b"yk_decode_output_resampled_device" in L.yk_last_error(fresh._h)
        assert int(batch(fresh._h, None, None, p, ow, oh, row, 0, row * oh, 3, 255)) == YK_ERR_STATE and b"yk_decode_output_resampled_batch_device" in L.yk_last_error(fresh._h)
    finally:
        fresh.close()
    refs = BW.batch_references(w, h, kind, n)
    # a single image: no rectangles to set; the batch call refuses a window
    ref, key = _refs(w, h, kind)
    dec.begin(w, h)
    assert int(setr(dec._h, tab(good_rects))) == YK_ERR_STATE
    dec.set_window(3, 5, 101, 97, px=True)
    _decode(dec, ref, key, "all_pass")
    assert int(batch(dec._h, None, None, p, ow, oh, row, 0, row * oh, 3, 255)) == YK_ERR_STATE and b"window" in L.yk_last_error(dec._h)
    assert int(single(dec._h, None, None, 0, p, ow, oh, row, 0, 4, -1)) == YK_ERR_STATE and b"alpha" in L.yk_last_error(dec._h)
    # a batch: bad rectangles leave it with neither rectangles nor windows
    dec.begin_batch(w, h, n)
    for bad in ([(-1, 0, 8, 8)] * 3, [(0, 0, 8, 8), (0, 0, 0, 8), (0, 0, 8, 8)], [(0, 0, 8, 8), (0, 0, 8, 8), (129, 0, 8, 8)], [(0, 257, 8, 8)] * 3, [(0, 0, 137, 8)] * 3):
        assert int(setr(dec._h, tab(bad))) == YK_ERR_BAD_ARG and b"yk_decode_set_batch_rects" in L.yk_last_error(dec._h), bad
    dec.set_batch_rects(good_rects)
    _decode_batch(dec, refs)
    assert int(setr(dec._h, tab(good_rects))) == YK_ERR_STATE and b"chunk" in L.yk_last_error(dec._h)     # after a chunk
    nan = float("nan")
    bad_norms = [NormC(0, f4(1, 1, 1, 1), f4(0, 0, 0, 0)), NormC(4, f4(1, 1, 1, 1), f4(0, 0, 0, 0)), NormC(1, f4(1, nan, 1, 1), f4(0, 0, 0, 0)),
                 NormC(1, f4(1, 1, 1, 1), f4(2.0 ** 101, 0, 0, 0))]
    flags = (C.c_uint8 * 3)(1, 0, 1)
    for args in [(C.byref(b), flags, p, ow, oh, ow * 6, 0, ow * 6 * oh, 3, 255) for b in bad_norms] + [
            (None, flags, None, ow, oh, row, 0, row * oh, 3, 255),                                                         # NULL
            (None, flags, p, 0, oh, row, 0, row * oh, 3, 255), (None, flags, p, ow, 0, row, 0, row * oh, 3, 255),          # sizes outside 1..16384
            (None, flags, p, 16385, 1, 16385 * 3, 0, 16385 * 3, 3, 255), (None, flags, p, 1, 16385, 3, 0, 16385 * 3, 3, 255), (None, flags, p, -1, oh, row, 0, row * oh, 3, 255),
            (None, flags, p, ow, oh, row - 1, 0, row * oh, 3, 255), (None, flags, p, ow, oh, row, 0, row * oh - 1, 3, 255),   # pitches too small
            (None, flags, p, ow, oh, ow - 1, ow * oh, ow * oh * 3, 3, 255), (None, flags, p, ow, oh, ow, ow * oh - 1, ow * oh * 3, 3, 255),
            (None, flags, p, ow, oh, ow, ow * oh, ow * oh * 3 - 1, 3, 255),
            (C.byref(good), flags, p + 1, ow, oh, ow * 6, 0, ow * 6 * oh, 3, 255), (C.byref(good), flags, p, ow, oh, ow * 6 + 1, 0, (ow * 6 + 1) * oh, 3, 255),   # misaligned
            (C.byref(f32), flags, p + 2, ow, oh, ow * 12, 0, ow * 12 * oh, 3, 255), (C.byref(f32), flags, p, ow, oh, ow * 12, 0, ow * 12 * oh + 2, 3, 255),
            (C.byref(good), flags, p, ow, oh, ow * 6 - 2, 0, ow * 6 * oh, 3, 255),
            (None, flags, p, ow, oh, row, 0, row * oh, 5, 255), (None, flags, p, ow, oh, ow * 4, 0, ow * 4 * oh, 4, 256), (None, flags, p, ow, oh, ow * 4, 0, ow * 4 * oh, 4, -2)]:
        assert int(batch(dec._h, *args)) == YK_ERR_BAD_ARG, args
        assert b"yk_decode_output_resampled_batch_device" in L.yk_last_error(dec._h)
    assert int(batch(dec._h, None, flags, p, ow, oh, ow * 4, 0, ow * 4 * oh, 4, -1)) == YK_ERR_STATE       # no decoded alpha planes
    assert int(single(dec._h, None, None, 0, p, ow, oh, row, 0, 3, 255)) == YK_ERR_STATE and b"rectangles" in L.yk_last_error(dec._h)
    # what §26 refuses under windows is refused under rectangles, naming them
    for call in (lambda: dec.image_batch_device(), lambda: dec.image_batch_windows_device(), lambda: dec.image_norm_batch_device("float16"),
                 lambda: dec.image_scaled_batch_device(1), lambda: dec.image_device()):
        with pytest.raises(Exception, match="rectangles"):
            call()
    assert bool((out == SENTINEL).all())                                      # nothing was written
    got = dec.image_resampled_batch_device((ow, oh), mirror=[1, 0, 1])        # a good call still gives the reference
    assert np.array_equal(got.cpu().numpy(), RR.batch_ref([r.rgb for r in refs], good_rects, (ow, oh), flags=[1, 0, 1]))
    # windows on the batch: the new batch call refuses
    dec.begin_batch(w, h, n)
    dec.set_batch_windows([(3, 5), (123, 253), (61, 59)], 13, 11, px=True)
    _decode_batch(dec, refs)
    assert int(batch(dec._h, None, None, p, ow, oh, row, 0, row * oh, 3, 255)) == YK_ERR_STATE and b"windows" in L.yk_last_error(dec._h)
    assert int(single(dec._h, None, None, 0, p, ow, oh, row, 0, 3, 255)) == YK_ERR_STATE
    # a prepared image has no resampled output
    from tests.test_gpu_decode_prepared import _prepare
    from tests.test_gpu_decode_prepared import _refs as _prepared_refs
    pref, calls = _prepared_refs(w, h, kind)
    _prepare(dec, w, h, calls)
    assert int(single(dec._h, None, None, 0, p, ow, oh, row, 0, 3, 255)) == YK_ERR_STATE and b"prepared" in L.yk_last_error(dec._h)
    assert bool((out == SENTINEL).all())
    # afterwards the handle decodes correctly
    dec.begin_batch(w, h, n)
    _decode_batch(dec, refs)
    assert np.array_equal(dec.image_batch_device().cpu().numpy(), np.stack([r.rgb for r in refs]))


# ---- 8: .yaik files --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files():
    from yaik_amd import files as F
    F.set_device_palette(False)
    yield F
    F.set_device_palette(False)


def test_files_equal_the_reference_of_the_whole_file_decode(files):
    from tests.golden.make_golden import PARTIAL
    from tests.test_gpu_decode_files_windows import _analog_alpha, _frames, _plane_subset
    w = h = 128
    rng = np.random.default_rng(128)
    rgb = _frames(w, h, "mixed", 3, False)
    rgba = np.stack([np.concatenate([rgb[f], _analog_alpha(w, h, rng)[..., None]], axis=2) for f in range(3)])
    fixture = np.ascontiguousarray(PARTIAL["pp_planemix128_rgb"]().astype(np.uint8).transpose(1, 2, 0))
    fallback = _plane_subset(files.encode_file_device(fixture))              # a plane-subset stream: the batch planner hands it to the single-image chain
    plain = [files.encode_file_device(rgba[f], emit_alpha=True) for f in range(3)]
    mixed = [plain[0], fallback, plain[2], files.encode_file_device(rgb[1])]
    all_rects = [(67, 59, 1, 1), (3, 5, 101, 97), (0, 0, 128, 128), (121, 122, 6, 5)]
    for strs, fallbacks in ((plain, 0), (mixed, 1)):
        n = len(strs)
        whole = files.decode_files_device(strs, channels=4).cpu().numpy()
        assert files.last_batch_info()["fallbacks"] == fallbacks
        flags, rects = RR.FLAGS[:n], all_rects[:n]
        for dtype in ELEMS:
            for size, channels, planar in (((13, 11), 4, False), ((7, 3), 3, True)):
                want = RR.batch_ref([whole[f][..., :channels] for f in range(n)], rects, size, dtype, SCALE, BIAS, flags)
                want = np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if planar else want
                raw, view, mask = _padded(dtype, want.shape, planar, True)
                assert files.decode_files_resampled_device(strs, size, rects=rects, mirror=flags, out=view, channels=channels, planar=planar, **_norm(dtype)) is view
                assert files.last_batch_info()["fallbacks"] == fallbacks
                assert np.array_equal(_bits(view, dtype), want), (fallbacks, dtype, size)
                assert bool((raw[~mask] == SENTINEL).all())
        got = files.decode_files_resampled_device(strs, (56, 40))            # whole frames
        assert np.array_equal(got.cpu().numpy(), RR.batch_ref([whole[f][..., :3] for f in range(n)], [(0, 0, w, h)] * n, (56, 40)))
    from yaik_amd.files import ERROR_NAMES, YaikFileError
    with pytest.raises(ValueError):                                          # a rectangle outside the image: Python says so first
        files.decode_files_resampled_device(plain, (13, 11), rects=[(0, 0, 8, 8), (124, 0, 8, 8), (0, 0, 8, 8)])
    H = files.host_lib()
    bufs = [files._buffer(s) for s in plain]
    ptrs = (C.c_void_p * 3)(*[b.ctypes.data for b in bufs])
    lens = (C.c_uint32 * 3)(*[b.size for b in bufs])
    torch = _torch()
    out = torch.full((3 * 13 * 11 * 3,), SENTINEL, dtype=torch.uint8, device="cuda")
    bad = (C.c_int * 12)(0, 0, 8, 8, 124, 0, 8, 8, 0, 0, 8, 8)               # ... and the library before a slot is taken
    assert not H.YAIK_DecodeImagesResampledToDevice(files.library(), ptrs, lens, 3, out.data_ptr(), 39, 0, 39 * 11, 3, 4, None, bad, 13, 11, None, None)
    assert ERROR_NAMES[H.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX" and bool((out == SENTINEL).all())
    assert tuple(files.decode_files_resampled_device(plain, (9, 9), dtype="float32").shape) == (3, 9, 9, 3)     # and the slot is free


# ---- 9: the existing calls after the new ones ------------------------------------------------------------------------------------------------------
def test_existing_calls_give_the_same_bytes_after_the_new_calls(dec, oracle_built):
    torch = _torch()
    w, h, kind, n = 136, 264, "mixed", 3
    refs = BW.batch_references(w, h, kind, n)
    origins = [(3, 5), (123, 253), (61, 59)]
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, 13, 11, px=True)
    _decode_batch(dec, refs)
    win = dec.image_batch_windows_device().clone()
    nrm = dec.image_norm_batch_device("bfloat16", scale=SCALE, bias=BIAS, mirror=[1, 1, 0]).clone()
    _begin_rects(dec, refs, RR.RECT_SETS[(w, h)]["mixed_a"])
    dec.synchronize()
    dec.stage_ms(YK_STAGE_DEC_DETILE)
    for dtype in ELEMS:
        dec.image_resampled_batch_device((56, 40), mirror=[1, 0, 1], **_norm(dtype))
    dec.synchronize()
    assert dec.stage_ms(YK_STAGE_DEC_DETILE)[1] == len(ELEMS)                # one de-tile interval per call
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, 13, 11, px=True)
    _decode_batch(dec, refs)
    assert torch.equal(dec.image_batch_windows_device(), win) and np.array_equal(win.cpu().numpy(), BW.crops(refs, (13, 11), origins))
    assert np.array_equal(NR.bits(dec.image_norm_batch_device("bfloat16", scale=SCALE, bias=BIAS, mirror=[1, 1, 0])), NR.bits(nrm))
    dec.begin_batch(w, h, n)
    _decode_batch(dec, refs)
    assert np.array_equal(dec.image_batch_device().cpu().numpy(), np.stack([r.rgb for r in refs]))
    ref, key = _refs(w, h, kind)
    dec.begin(w, h)
    _decode(dec, ref, key, "all_pass")
    dec.image_resampled_device((13, 11))
    assert np.array_equal(dec.image_device().cpu().numpy(), ref.rgb)
