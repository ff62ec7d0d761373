"""A window of every frame of a batch on the GPU (yk_decode_set_batch_windows): with windows set, frame f of
image_batch_windows_device equals the crop of the oracle's whole decode of frame f at frame f's origin, bit for bit, on the batches and window
sets of tests/batch_window_cases.py; tile4x4Mask stays whole per frame, the planes outside a frame's window rounded to 64 are not written, the
rectangle table of one batch is never read by the kernels of another, and the calls that need whole frames refuse while windows are set."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_window_cases as BC
from tests import window_cases as WC

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
YK_ERR_BAD_ARG, YK_ERR_STATE = -2, -4
YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE = 3, 4, 5


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
def one():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


_DEVICE = {}


def _frame_calls(ref):
    """the oracle's streams of one frame in device memory as a call list of decode_batch_streams / decode_streams: all seven passes (an empty
    pass: its all-zero bitmap, no colours), then the 1-D chunk; uploaded once per Reference and kept alive here"""
    torch = _torch()
    if id(ref) not in _DEVICE:
        keep, calls = [ref], []
        for sx, sy, cnt, bm, rgb in ref.passes:
            tb = torch.from_numpy(np.ascontiguousarray(bm)).cuda()
            tr = torch.from_numpy(np.concatenate([rgb, np.zeros(16, np.uint8)])).cuda()
            keep += [tb, tr]
            calls.append(("g", sx, sy, tb.data_ptr(), bm.size, tr.data_ptr() if rgb.size else 0, rgb.size))
        tt = torch.from_numpy(np.concatenate([ref.typ, np.zeros(16, np.uint8)])).cuda()
        tp = torch.from_numpy(np.concatenate([ref.pix, np.zeros(16, np.uint8)])).cuda()
        keep += [tt, tp]
        calls.append(("1", tt.data_ptr() if ref.typ.size else 0, ref.typ.size, tp.data_ptr() if ref.pix.size else 0, ref.pix.size))
        torch.cuda.synchronize()
        _DEVICE[id(ref)] = (keep, calls)
    return _DEVICE[id(ref)][1]


def _decode_batch(d, refs, gradients_only=False, sync=True):
    frames = [[c for c in _frame_calls(r) if c[0] == "g" or not gradients_only] for r in refs]
    d.decode_batch_streams(frames, sync=sync, remap_range=0)


def _windowed(d, refs, size, origins, sync=True):
    """begin_batch + set_batch_windows + the chunks of every frame"""
    d.begin_batch(refs[0].w, refs[0].h, len(refs))
    d.set_batch_windows(origins, *size)
    _decode_batch(d, refs, sync=sync)


def _alpha_entries(w, h, n, seed):
    """mode 6 (8-bit) 'ALPM' entries of n frames, each with its own box and bytes (never 255, what a pixel outside the box gets)"""
    rng = np.random.default_rng(seed)
    entries = []
    for f in range(n):
        bx, by = (8 * (f % 2), 8 * ((f // 2) % 2)) if w > 16 and h > 16 else (0, 0)
        bw, bh = w - bx, h - by
        pay = rng.integers(1, 255, bw * bh).astype(np.uint8)
        entries.append((6, (bx, by, bw, bh), pay))
    return entries


def _padded_batch(torch, n, wh, ww, c, planar, extra_row=11, extra_plane=13, extra_frame=29, offset=3):
    row = (ww if planar else ww * c) + extra_row
    if planar:
        plane = row * wh + extra_plane
        frame = plane * c + extra_frame
        shape, strides = (n, c, wh, ww), (frame, plane, row, 1)
    else:
        frame = row * wh + extra_frame
        shape, strides = (n, wh, ww, c), (frame, row, c, 1)
    size = offset + frame * n + 64
    buf = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
    mask = torch.zeros(size, dtype=torch.bool, device="cuda")
    torch.as_strided(mask, shape, strides, offset).fill_(True)
    return buf, torch.as_strided(buf, shape, strides, offset), mask


def _ids(v):
    return str(v) if isinstance(v, (str, int)) else ""


# ---- crop equality: every window set of every batch, every layout ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,n,name,size,origins", BC.all_batch_sets(), ids=_ids)
def test_every_window_equals_the_oracle_crop(dec, oracle_built, w, h, kind, n, name, size, origins):
    torch = _torch()
    refs = BC.batch_references(w, h, kind, n)
    ww, wh = size
    dec.begin_batch(w, h, n)
    assert dec.batch_windows is None
    dec.set_batch_windows(np.asarray(origins, dtype=np.int64), ww, wh)
    got_o, got_w, got_h = dec.batch_windows
    assert got_o.tolist() == [list(o) for o in origins] and (got_w, got_h) == size
    dec.decompress_alpha_batch(_alpha_entries(w, h, n, seed=w + h + n), 255, sync=False)     # the planes stay whole; a window reads them at its offset
    _decode_batch(dec, refs)
    alpha = []
    for f in range(n):
        dec.select_frame(f)
        alpha.append(dec.alpha_plane())
        # the marks are whole and exact for every frame, the planes exact inside the frame's window
        assert np.array_equal(dec.tile4x4(), refs[f].tile4), f
        x0, y0 = origins[f]
        inside = np.s_[:, y0 // 8:(y0 + wh) // 8, x0 // 8:(x0 + ww) // 8]
        assert np.array_equal(WC.tiles_of(dec.planes(), w, h)[inside], WC.tiles_of(refs[f].planes, w, h)[inside]), f
    rgb = BC.crops(refs, size, origins)
    a_crop = np.stack([alpha[f][y0:y0 + wh, x0:x0 + ww] for f, (x0, y0) in enumerate(origins)])
    assert a_crop.min() < 255
    for channels, kw, a_want in ((3, {}, None), (4, {"alpha": 77}, np.full((n, wh, ww), 77, np.uint8)), (4, {"alpha_from_planes": True}, a_crop)):
        want = rgb if a_want is None else np.concatenate([rgb, a_want[..., None]], axis=3)
        for planar in (False, True):
            exp = torch.from_numpy(np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if planar else want).cuda()
            got = dec.image_batch_windows_device(channels=channels, planar=planar, **kw)
            assert got.dtype == torch.uint8 and torch.equal(got, exp), (channels, kw, planar)
            buf, view, mask = _padded_batch(torch, n, wh, ww, channels, planar)
            assert dec.image_batch_windows_device(out=view, channels=channels, planar=planar, **kw) is view
            assert torch.equal(view, exp), (channels, kw, planar, "padded")
            assert (buf[~mask] == SENTINEL).all(), (channels, kw, planar, "a byte outside the pixels changed")
    with pytest.raises(ValueError, match="windows need"):
        dec.image_batch_windows_device(out=torch.empty((n, wh + 8, ww, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="windows need"):
        dec.image_batch_windows_device(out=torch.empty((n + 1, wh, ww, 3), dtype=torch.uint8, device="cuda"))


# ---- frame swap: the table is indexed by the frame ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,n", [b for b in BC.BATCHES if b[2] == "mixed"], ids=_ids)
def test_windows_permuted_among_the_frames_give_the_permuted_crops(dec, oracle_built, w, h, kind, n):
    refs = BC.batch_references(w, h, kind, n)
    for name, size, origins in BC.window_sets(w, h):
        if name in BC.SAME_ORIGIN:
            continue
        perm = origins[1:] + origins[:1]
        _windowed(dec, refs, size, perm)
        got = dec.image_batch_windows_device().cpu().numpy()
        assert np.array_equal(got, BC.crops(refs, size, perm)), name
        assert not np.array_equal(got, BC.crops(refs, size, origins)), name     # ... which the unpermuted table would not have given


# ---- the not-written guarantee, per frame ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,n", [b for b in BC.BATCHES if b[2] == "mixed"], ids=_ids)
def test_planes_outside_each_frames_blocks_keep_the_previous_batch(dec, oracle_built, w, h, kind, n):
    refs_a, refs_b = BC.batch_references(w, h, kind, n), BC.batch_references(w, h, kind, n, second=True)
    for name, size, origins in BC.window_sets(w, h):
        if name in BC.SAME_ORIGIN:
            continue
        dec.begin_batch(w, h, n)
        _decode_batch(dec, refs_a)
        dec.begin_batch(w, h, n)
        dec.set_batch_windows(origins, *size)
        _decode_batch(dec, refs_b)
        for f, (x0, y0) in enumerate(origins):
            dec.select_frame(f)
            got = WC.tiles_of(dec.planes(), w, h)
            a, b = WC.tiles_of(refs_a[f].planes, w, h), WC.tiles_of(refs_b[f].planes, w, h)
            inside = np.s_[:, y0 // 8:(y0 + size[1]) // 8, x0 // 8:(x0 + size[0]) // 8]
            assert np.array_equal(got[inside], b[inside]), (name, f)
            outside = WC.outside_rounded(w, h, (x0, y0) + size)
            assert outside.any()
            assert np.array_equal(got[:, outside], a[:, outside]), (name, f, "a tile outside the window's 64-blocks was written")
            assert (a[:, outside] != b[:, outside]).any()                    # the two batches differ there, so a write would show
            assert np.array_equal(dec.tile4x4(), refs_b[f].tile4), (name, f)
        assert np.array_equal(dec.image_batch_windows_device().cpu().numpy(), BC.crops(refs_b, size, origins)), name


def test_settle_zeroes_the_unmarked_cells_of_each_frames_window_only(dec, oracle_built):
    """gradient chunks only, then an output: what no chunk wrote reads as zero inside each window, as in the whole-batch flow, and the planes
    outside the windows' blocks still hold the batch before"""
    w, h, kind, n = 520, 264, "mixed", 4
    refs_a, refs_b = BC.batch_references(w, h, kind, n), BC.batch_references(w, h, kind, n, second=True)
    size, origins = BC.WINDOW_SETS[(w, h)]["scan_block"]
    dec.begin_batch(w, h, n)
    _decode_batch(dec, refs_b, gradients_only=True)
    whole = dec.image_batch_device().cpu().numpy()                           # B's gradient tiles, zeros elsewhere
    dec.begin_batch(w, h, n)
    _decode_batch(dec, refs_a)
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, *size)
    _decode_batch(dec, refs_b, gradients_only=True)
    got = dec.image_batch_windows_device().cpu().numpy()
    for f, (x0, y0) in enumerate(origins):
        assert np.array_equal(got[f], whole[f, y0:y0 + size[1], x0:x0 + size[0]]), f
        dec.select_frame(f)
        outside = WC.outside_rounded(w, h, (x0, y0) + size)
        assert np.array_equal(WC.tiles_of(dec.planes(), w, h)[:, outside], WC.tiles_of(refs_a[f].planes, w, h)[:, outside]), f


# ---- empty frames between ordinary ones -----------------------------------------------------------------------------------------------------
def test_frames_without_gradient_tiles_or_without_1d_bytes(dec, oracle_built):
    w, h, frames = BC.EMPTY_BATCH
    size, origins = BC.EMPTY_WINDOWS
    refs = [BC.reference(w, h, kind, f) for kind, f in frames]
    assert not any(cnt for _, _, cnt, _, _ in refs[1].passes) and refs[2].typ.size == 0 and refs[2].pix.size == 0
    _windowed(dec, refs, size, origins)
    assert np.array_equal(dec.image_batch_windows_device().cpu().numpy(), BC.crops(refs, size, origins))
    for f in range(len(refs)):
        dec.select_frame(f)
        assert np.array_equal(dec.tile4x4(), refs[f].tile4), f


# ---- single-image equivalence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,n", BC.BATCHES + [(136, 264, "mixed", 1)], ids=_ids)
def test_every_frame_equals_the_single_image_window_decode(dec, one, oracle_built, w, h, kind, n):
    torch = _torch()
    refs = BC.batch_references(w, h, kind, n)
    for name, size, origins in BC.window_sets(w, h):
        origins = origins[:n]
        _windowed(dec, refs, size, origins)
        got = dec.image_batch_windows_device(channels=4, alpha=9)
        for f, (x0, y0) in enumerate(origins):
            one.begin(w, h)
            one.set_window(x0, y0, *size)
            one.decode_streams([c for c in _frame_calls(refs[f]) if c[0] == "1" or c[6]], remap_range=0)
            assert torch.equal(got[f], one.image_window_device(channels=4, alpha=9)), (name, f)


# ---- the table's lifetime -------------------------------------------------------------------------------------------------------------------
def test_two_windowed_batches_back_to_back_then_whole_decodes(dec, oracle_built):
    w, h, kind, n = 520, 264, "mixed", 4
    refs_a, refs_b = BC.batch_references(w, h, kind, n), BC.batch_references(w, h, kind, n, second=True)
    size, origins = BC.WINDOW_SETS[(w, h)]["scan_block"]
    other = origins[2:] + origins[:2]
    for r in refs_a + refs_b:
        _frame_calls(r)                                                      # uploaded before the queue starts: nothing below waits for the host
    dec.synchronize()
    _windowed(dec, refs_a, size, origins, sync=False)
    first = dec.image_batch_windows_device()
    _windowed(dec, refs_b, size, other, sync=False)                          # queued behind the first batch's kernels, which read the first table
    second = dec.image_batch_windows_device()
    dec.synchronize()
    assert np.array_equal(first.cpu().numpy(), BC.crops(refs_a, size, origins))
    assert np.array_equal(second.cpu().numpy(), BC.crops(refs_b, size, other))
    # begin_batch cleared the windows: a whole batch, then a plain begin, on the same handle
    dec.begin_batch(w, h, n)
    assert dec.batch_windows is None
    _decode_batch(dec, refs_a)
    assert np.array_equal(dec.image_batch_device().cpu().numpy(), np.stack([r.rgb for r in refs_a]))
    for f in range(n):
        dec.select_frame(f)
        assert np.array_equal(dec.planes(), refs_a[f].planes), f
    dec.begin(w, h)
    dec.decode_streams([c for c in _frame_calls(refs_b[1]) if c[0] == "1" or c[6]], remap_range=0)
    assert np.array_equal(dec.image_device().cpu().numpy(), refs_b[1].rgb)
    assert np.array_equal(dec.planes(), refs_b[1].planes)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _err(d):
    from yaik_amd._lib import lib
    return lib().yk_last_error(d._h).decode()


def _xy(origins):
    flat = [v for o in origins for v in o]
    return (C.c_int * len(flat))(*flat)


def test_set_batch_windows_state_and_argument_refusals(dec, oracle_built):
    from yaik_amd._lib import YaikError, lib
    from yaik_amd.decoder import HipTileDecoder
    L = lib()
    w, h, kind, n = 136, 264, "mixed", 3
    refs = BC.batch_references(w, h, kind, n)
    size, origins = BC.WINDOW_SETS[(w, h)]["four_blocks"]
    good = _xy(origins)
    fresh = HipTileDecoder(0)
    try:
        assert L.yk_decode_set_batch_windows(fresh._h, good, *size) == YK_ERR_STATE and "yk_decode_begin_batch" in _err(fresh)      # before any begin
        assert L.yk_decode_output_batch_windows_device(fresh._h, 16, 64, 0, 64 * 8, 3, 255) == YK_ERR_STATE and "begin" in _err(fresh)
        fresh.begin(w, h)
        assert L.yk_decode_set_batch_windows(fresh._h, good, *size) == YK_ERR_STATE and "yk_decode_begin_batch" in _err(fresh)      # a single image
        assert L.yk_decode_set_batch_windows(fresh._h, None, 0, 0) == YK_ERR_STATE
        with pytest.raises(YaikError, match="yk_decode_begin_batch"):
            fresh.set_batch_windows(origins[:1], *size)
        assert fresh.batch_windows is None
        fresh.set_window(0, 0, 8, 8)                                         # the handle is usable: a single image takes its own window
    finally:
        fresh.close()
    dec.begin_batch(w, h, n)
    assert L.yk_decode_set_window(dec._h, 0, 0, 8, 8) == YK_ERR_STATE and "batch" in _err(dec)           # stays refused on a batch
    for ww, wh in ((12, 8), (8, 12), (0, 8), (8, 0), (-8, -8), (144, 8), (8, 272), (4, 4)):
        assert L.yk_decode_set_batch_windows(dec._h, _xy([(0, 0)] * n), ww, wh) == YK_ERR_BAD_ARG, (ww, wh)
        assert "yk_decode_set_batch_windows" in _err(dec) and "multiples of 8" in _err(dec)
    for f in range(n):                                                       # one frame's origin wrong at a time, the others valid
        for bad in ((4, 0), (0, 4), (-8, 0), (0, -8), (136 - 24, 0), (0, 264 - 24), (136, 0), (2 ** 31 - 8, 0)):
            o = list(origins)
            o[f] = bad
            assert L.yk_decode_set_batch_windows(dec._h, _xy(o), *size) == YK_ERR_BAD_ARG, (f, bad)
    assert L.yk_decode_set_batch_windows(dec._h, None, *size) == YK_ERR_BAD_ARG and "NULL" in _err(dec)
    # a refused argument leaves the batch without windows, also when windows were set before it
    dec.set_batch_windows(origins, *size)
    assert L.yk_decode_set_batch_windows(dec._h, _xy([(0, 0)] * n), 12, 8) == YK_ERR_BAD_ARG
    out = _torch().full((n, h, w, 3), SENTINEL, dtype=_torch().uint8, device="cuda")
    assert L.yk_decode_output_batch_windows_device(dec._h, out.data_ptr(), w * 3, 0, w * h * 3, 3, 255) == YK_ERR_STATE and "no windows" in _err(dec)
    # Python refuses bad arguments before any library call
    dec.begin_batch(w, h, n)
    for bad_o, exc in ((origins[:2], ValueError), (origins + [(0, 0)], ValueError), ([(4, 0)] + origins[1:], ValueError), ([(120, 0)] + origins[1:], ValueError),
                       ([(0.0, 0)] + origins[1:], TypeError), (np.zeros((n, 3), np.int64), TypeError), (np.zeros((n, 2), np.float32), TypeError)):
        with pytest.raises(exc):
            dec.set_batch_windows(bad_o, *size)
    with pytest.raises(ValueError):
        dec.set_batch_windows(origins, 32, 12)
    with pytest.raises(ValueError, match="set_batch_windows"):
        dec.image_batch_windows_device()
    assert dec.batch_windows is None
    # clearing, and the clear of every begin
    dec.set_batch_windows(origins, *size)
    dec.set_batch_windows(None, 0, 0)
    assert dec.batch_windows is None
    dec.set_batch_windows(origins, *size)
    dec.begin_batch(w, h, n)
    assert dec.batch_windows is None
    _decode_batch(dec, refs)
    assert np.array_equal(dec.image_batch_device().cpu().numpy(), np.stack([r.rgb for r in refs]))       # whole frames: no window survived
    # after a chunk of the batch: too late, for windows and for clearing them
    assert L.yk_decode_set_batch_windows(dec._h, good, *size) == YK_ERR_STATE and "chunk" in _err(dec)
    assert L.yk_decode_set_batch_windows(dec._h, None, 0, 0) == YK_ERR_STATE
    for first in ("gradient", "1d"):
        dec.begin_batch(w, h, n)
        frames = [[c for c in _frame_calls(r) if (c[0] == "g") == (first == "gradient")] for r in refs]
        dec.decode_batch_streams(frames, remap_range=0)
        assert L.yk_decode_set_batch_windows(dec._h, good, *size) == YK_ERR_STATE, first
    # the 'ALPM' planes are whole and no chunk of the planes: the windows may follow them
    dec.begin_batch(w, h, n)
    dec.decompress_alpha_batch(_alpha_entries(w, h, n, seed=9), 255)
    dec.set_batch_windows(origins, *size)
    _decode_batch(dec, refs)
    assert np.array_equal(dec.image_batch_windows_device().cpu().numpy(), BC.crops(refs, size, origins))      # ... and the handle decodes correctly


def test_whole_frame_calls_refuse_while_windows_are_set(dec, oracle_built):
    torch = _torch()
    from yaik_amd._lib import YaikError, lib
    L = lib()
    w, h, kind, n = 136, 264, "mixed", 3
    refs = BC.batch_references(w, h, kind, n)
    size, origins = BC.WINDOW_SETS[(w, h)]["four_blocks"]
    ww, wh = size
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, ww, wh)
    dec.decompress_alpha_batch(_alpha_entries(w, h, n, seed=11), 255)
    _decode_batch(dec, refs)
    ok = dec.image_batch_windows_device(channels=4, alpha_from_planes=True)
    src = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    calls = [lambda: dec.image_batch_device(), lambda: dec.image_batch_device(channels=4, alpha_from_planes=True),
             lambda: dec.image_scaled_batch_device(1), lambda: dec.image_scaled_batch_device(0), lambda: dec.image_mipchain_batch_device(0, 2),
             lambda: dec.compare_batch_device(src), lambda: dec.image_device(), lambda: dec.image_window_device(), lambda: dec.image(),
             lambda: dec.image_scaled_device(1), lambda: dec.compare_device(src[0]),
             lambda: dec.decode_streams([c for c in _frame_calls(refs[0]) if c[0] == "g" and c[6]], remap_range=0),
             lambda: dec.decode_streams([c for c in _frame_calls(refs[0]) if c[0] == "g" and c[6]], per_pass=True, remap_range=0),
             lambda: dec.decode_streams([c for c in _frame_calls(refs[0]) if c[0] == "1"], remap_range=0),
             lambda: dec.decompress_1d(refs[0].typ, refs[0].pix)]
    for f in (0, n - 1):
        dec.select_frame(f)                                                  # stays allowed
        for k, call in enumerate(calls):
            with pytest.raises(YaikError, match="yk_decode_set_batch_windows") as e:
                call()
            assert f"error {YK_ERR_STATE}" in str(e.value), k
    assert L.yk_decode_split_masks(dec._h) == YK_ERR_STATE                  # a batch of several frames refuses it anyway
    # the refusals wrote nothing and left everything as it was: the output, the marks, the planes and the alpha planes stay readable
    assert torch.equal(dec.image_batch_windows_device(channels=4, alpha_from_planes=True), ok)
    assert np.array_equal(ok.cpu().numpy()[..., :3], BC.crops(refs, size, origins))
    for f in range(n):
        dec.select_frame(f)
        assert np.array_equal(dec.tile4x4(), refs[f].tile4) and dec.planes().shape == (3, (w // 8) * (h // 8) * 64) and dec.alpha_plane().shape == (h, w)
    # layouts that do not hold the windows are refused by the library too, and write nothing
    out = torch.full((n, wh, ww, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    p, fb = out.data_ptr(), ww * wh * 4
    for args in ((None, ww * 3, 0, fb, 3, 255), (p, ww * 3 - 1, 0, fb, 3, 255), (p, ww * 3, 0, ww * wh * 3 - 1, 3, 255), (p, ww * 3, 0, fb, 5, 255),
                 (p, ww * 4, 0, fb, 4, 256), (p, ww * 4, 0, fb, 4, -2), (p, ww, ww * wh - 1, fb, 3, 255), (p, ww, ww * wh, 3 * ww * wh - 1, 3, 255)):
        assert L.yk_decode_output_batch_windows_device(dec._h, *args) == YK_ERR_BAD_ARG, args
        assert "yk_decode_output_batch_windows_device" in _err(dec)
    assert (out == SENTINEL).all()
    # alpha from the planes needs the planes of this batch
    _windowed(dec, refs, size, origins)
    assert L.yk_decode_output_batch_windows_device(dec._h, p, ww * 4, 0, fb, 4, -1) == YK_ERR_STATE and "alpha" in _err(dec)
    assert (out == SENTINEL).all()
    assert np.array_equal(dec.image_batch_windows_device().cpu().numpy(), BC.crops(refs, size, origins))


# ---- timers ---------------------------------------------------------------------------------------------------------------------------------
def test_a_windowed_batch_records_one_interval_per_stage(dec, oracle_built):
    w, h, kind, n = 136, 264, "mixed", 3
    refs = BC.batch_references(w, h, kind, n)
    size, origins = BC.WINDOW_SETS[(w, h)]["row"]
    stages = (YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE)
    dec.synchronize()
    for st in stages:
        dec.stage_ms(st)                                                     # fold what earlier tests left
    for rep in (1, 2):
        for _ in range(rep):
            _windowed(dec, refs, size, origins)
            dec.image_batch_windows_device()
        dec.synchronize()
        got = [dec.stage_ms(st) for st in stages]
        assert [c for _, c in got] == [rep] * 3 and all(ms > 0 for ms, _ in got)


# ---- one mid-size case from the encoder -----------------------------------------------------------------------------------------------------
def test_16_frames_of_512_random_224_crops_from_the_encoder(dec):
    torch = _torch()
    from yaik_amd.encoder import HipTileEncoder
    from yaik_amd.synth import synth_planes
    n, s, ww = 16, 512, 224
    rng = np.random.default_rng(512224)
    planes = np.stack([synth_planes(s, n_planes=3, seed=100 + f) for f in range(n)])
    frames = torch.from_numpy(np.ascontiguousarray(np.moveaxis(planes, 1, -1)).astype(np.uint8)).cuda()
    origins = [(int(rng.integers(0, (s - ww) // 8 + 1)) * 8, int(rng.integers(0, (s - ww) // 8 + 1)) * 8) for _ in range(n)]
    assert len(set(origins)) == n
    enc = HipTileEncoder(0)
    try:
        enc.set_batch_u8(frames)
        enc.encode_batch(3, False)
        dec.begin_batch(s, s, n)
        dec.decode_batch_from_encoder(enc)
        whole = dec.image_batch_device().clone()
        marks = []
        for f in range(n):
            dec.select_frame(f)
            marks.append(dec.tile4x4())
        dec.begin_batch(s, s, n)
        dec.decode_batch_from_encoder(enc, windows=(origins, ww, ww))
        assert dec.batch_windows[1:] == (ww, ww)
        got = dec.image_batch_windows_device()
        assert tuple(got.shape) == (n, ww, ww, 3)
        for f, (x0, y0) in enumerate(origins):
            assert torch.equal(got[f], whole[f, y0:y0 + ww, x0:x0 + ww]), f
            dec.select_frame(f)
            assert np.array_equal(dec.tile4x4(), marks[f]), f
    finally:
        dec.synchronize()
        enc.close()
