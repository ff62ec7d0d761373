"""The mask modes 2 / 3 of 'ALPM' in a batch: yk_decode_alpha_mask_batch_device + yk_decode_alpha_batch_status (HipTileDecoder.
decompress_alpha_batch with five-tuple entries, alpha_batch_status).  Every frame's plane is compared, bit for bit, with two references: the
single-image path on a second decoder (decompress_1bit_tiled + decompress_alpha) and the numpy restatement tests/alpha_ref.py."""
import ctypes as C

import numpy as np
import pytest

from tests import alpha_ref as R
from yaik_amd._lib import lib
from yaik_amd.decoder import HipTileDecoder, pack_alpha_batch

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_ERR_RANGE = -2, -4, -5
SENTINEL = 0xA5


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dec1():
    d = HipTileDecoder(0)
    yield d
    d.close()


def _pixel_box(tile_box):
    return tuple(int(v) * 16 for v in tile_box)


def _selected(bbox, bits, tile_box):
    """how many pixels of the alpha box the mask selects, by the restatement's own rule (R.decode reads the same positions)"""
    tx, ty, tw, th = tile_box
    m = R.swizzled_mask(bits, tw, th)
    bx, by, bw, bh = bbox
    stride = tw * 16
    base = ((bx - tx * 16) + stride * (by - ty * 16)) & 0xFFFFFFFF
    r, c = np.mgrid[0:bh, 0:bw]
    pos = (base + stride * r.astype(np.int64) + c) & 0xFFFFFFFF
    inside = (pos >> 3) < m.size
    sel = np.zeros((bh, bw), bool)
    sel[inside] = ((m[pos[inside] >> 3] >> (pos[inside] & 7)) & 1) != 0
    return int(sel.sum())


def _masked(rng, mode, bbox, tile_box, bits=None, short=0):
    """(mode, bbox, payload, bits, tile box): random tile bits unless given, a random payload of exactly the needed length minus `short`"""
    tw, th = tile_box[2], tile_box[3]
    if bits is None:
        bits = np.packbits(rng.integers(0, 2, tw * th).astype(np.uint8), bitorder="little")
    need = (_selected(bbox, bits, tile_box) * 6 + 7) // 8
    return (mode, tuple(bbox), rng.integers(0, 256, need - short, dtype=np.uint8), np.asarray(bits, np.uint8), tuple(tile_box))


def _want(e, w, h, fill):
    if e is None:
        return np.full((h, w), fill, np.uint8)
    if len(e) == 5:
        return R.decode(e[0], e[1], e[2], w, h, R.swizzled_mask(e[3], e[4][2], e[4][3]), _pixel_box(e[4]), reference_1bit=False)
    return R.decode(e[0], e[1], e[2], w, h, reference_1bit=False)


def _single(dec1, e, w, h):
    """the single-image path: yk_decode_mask, then yk_decode_alpha with the decoded mask and its box in pixels"""
    dec1.begin(w, h)
    if len(e) == 5:
        mask = dec1.decompress_1bit_tiled(e[3], e[4][2], e[4][3])
        return dec1.decompress_alpha(e[0], e[1], e[2], mask, _pixel_box(e[4]))
    return dec1.decompress_alpha(e[0], e[1], e[2])


def _check(dec, dec1, ent, w, h, fill=255, single=True):
    dec.begin_batch(w, h, len(ent))
    dec.decompress_alpha_batch(ent, fill)
    planes = []
    for f, e in enumerate(ent):
        dec.select_frame(f)
        got = dec.alpha_plane()
        np.testing.assert_array_equal(got, _want(e, w, h, fill), err_msg=f"frame {f}: restatement")
        if e is not None and single:
            np.testing.assert_array_equal(got, _single(dec1, e, w, h), err_msg=f"frame {f}: single-image path")
        planes.append(got)
    return planes


def _five_72x40(rng):
    """72 x 40 (W = 8 mod 16, a 5 x 3 tile grid), modes [3, -1, 2, 6, 3]: mask boxes narrower than the image, alpha boxes off the mask origin"""
    w, h = 72, 40
    return [_masked(rng, 3, (20, 5, 40, 30), (1, 0, 3, 2)),
            None,
            _masked(rng, 2, (4, 17, 64, 20), (0, 1, 4, 2)),
            (R.IS_8_BIT_FULL, (9, 3, 50, 31), rng.integers(0, 256, 50 * 31, dtype=np.uint8)),
            _masked(rng, 3, (36, 0, 36, 40), (2, 0, 2, 3))], w, h


def test_mixed_modes_narrow_masks(dec, dec1):
    ent, w, h = _five_72x40(np.random.default_rng(41))
    assert any(e is not None and len(e) == 5 and 0 < _selected(e[1], e[3], e[4]) < e[1][2] * e[1][3] for e in ent)
    _check(dec, dec1, ent, w, h, fill=93)
    assert dec.alpha_batch_status().tolist() == [0] * 5


def test_wide_box_empty_and_full_masks(dec, dec1):
    """a box 144 wide: three ballot steps per row; one mask selects nothing, one everything"""
    rng = np.random.default_rng(42)
    w, h, grid = 160, 48, (0, 0, 10, 3)
    none, every = np.zeros(4, np.uint8), np.packbits(np.ones(30, np.uint8), bitorder="little")
    ent = [_masked(rng, 3, (12, 2, 144, 44), grid),
           _masked(rng, 2, (16, 0, 144, 48), grid, bits=none),
           _masked(rng, 3, (0, 1, 144, 47), grid, bits=every)]
    assert ent[1][2].size == 0 and ent[2][2].size == 144 * 47 * 6 // 8
    planes = _check(dec, dec1, ent, w, h)
    assert not planes[1].any()
    assert dec.alpha_batch_status().tolist() == [0, 0, 0]


def test_scan_beyond_1024_rows(dec, dec1):
    rng = np.random.default_rng(43)
    w, h, grid = 16, 1056, (0, 0, 1, 66)
    ent = [_masked(rng, 3, (0, 8, 16, 1040), grid), _masked(rng, 2, (4, 16, 12, 1040), grid)]
    _check(dec, dec1, ent, w, h)
    assert dec.alpha_batch_status().tolist() == [0, 0]


def test_status_of_a_short_payload(dec, dec1):
    w, h = 72, 40
    box, grid = (20, 5, 40, 30), (1, 0, 3, 2)
    bits = np.packbits(np.array([1, 0, 1, 1, 1, 0], np.uint8), bitorder="little")
    for short in (0, 1):
        rng = np.random.default_rng(44)
        ent = [_masked(rng, 3, box, grid, bits=bits, short=short), (R.IS_8_BIT_FULL, (0, 0, 72, 40), rng.integers(0, 256, 72 * 40, dtype=np.uint8)),
               _masked(rng, 2, (4, 17, 64, 20), (0, 1, 4, 2))]
        assert _selected(box, bits, grid) > 0
        # the restatement reads missing bytes as 0, as the batch call does; the single-image call refuses a short payload
        _check(dec, dec1, ent, w, h, single=(short == 0))
        assert dec.alpha_batch_status().tolist() == [short, 0, 0]
    dec.decompress_alpha_batch([None, ent[1], None])                        # the three-tuple call behind it: nothing masked, nothing reported
    assert dec.alpha_batch_status().tolist() == [0, 0, 0]


def test_refusals_leave_the_planes(dec):
    torch = _torch()
    L = lib()
    rng = np.random.default_rng(45)
    w, h, n = 72, 40, 3                                                      # tile grid 5 x 3
    pay = rng.integers(0, 256, w * h, dtype=np.uint8)
    bits = np.full(4, 0xFF, np.uint8)
    dec.begin_batch(w, h, n)
    st = np.zeros(n, np.int32)
    assert L.yk_decode_alpha_batch_status(dec._h, st.ctypes.data) == YK_ERR_STATE       # no planes yet
    good = [(R.IS_8_BIT_FULL, (8, 4, 40, 30), pay[:1200]), None, _masked(rng, 3, (20, 5, 40, 30), (1, 0, 3, 2))]
    dec.decompress_alpha_batch(good, SENTINEL)
    want = [_want(e, w, h, SENTINEL) for e in good]

    def call(entries, masks=True, fill=255, null_bits=(), mip_bytes=None):
        pk = pack_alpha_batch(entries)
        stage = torch.from_numpy(pk.staging if pk.staging.size else np.zeros(16, np.uint8)).cuda()
        torch.cuda.synchronize()
        base = stage.data_ptr()
        ptrs = (C.c_void_p * n)(*[None if x is None else base + x[1] for x in pk.where])
        sizes = (C.c_size_t * n)(*[int(v) for v in pk.nbytes])
        if not masks:
            return L.yk_decode_alpha_batch_device(dec._h, pk.modes.ctypes.data, pk.bboxes.ctypes.data, ptrs, sizes, fill)
        where = pk.mip_where or [None] * n
        mptrs = (C.c_void_p * n)(*[None if o is None or f in null_bits else base + o for f, o in enumerate(where)])
        mb = [int(v) for v in (pk.mip_nbytes if pk.mip_nbytes is not None else np.zeros(n))]
        for f, v in (mip_bytes or {}).items():
            mb[f] = v
        boxes = np.ascontiguousarray(pk.mip_boxes if pk.mip_boxes is not None else np.zeros((n, 4), np.int32))
        return L.yk_decode_alpha_mask_batch_device(dec._h, pk.modes.ctypes.data, pk.bboxes.ctypes.data, ptrs, sizes, mptrs, (C.c_size_t * n)(*mb),
                                                   boxes.ctypes.data, fill)

    g0 = good[0]
    box, grid = (20, 5, 40, 30), (1, 0, 3, 2)
    # everything yk_decode_alpha_batch_device refuses
    assert call([g0, None, (R.IS_8_BIT_FULL, (60, 0, 16, 8), pay)]) == YK_ERR_BAD_ARG
    assert call([g0, None, (R.IS_1_BIT_FULL, (0, 0, 12, 4), pay)]) == YK_ERR_BAD_ARG
    assert call([g0, (R.IS_6_BIT_FULL, (0, 0, 10, 4), pay), None]) == YK_ERR_BAD_ARG
    assert call([g0, None, (0, (0, 0, 16, 16), pay)]) == YK_ERR_BAD_ARG
    assert call([g0, None, (7, (0, 0, 16, 16), pay)]) == YK_ERR_BAD_ARG
    assert call(good, fill=256) == YK_ERR_BAD_ARG
    assert call([g0, None, (R.IS_8_BIT_FULL, (0, 0, 16, 16), pay[:255])]) == YK_ERR_RANGE
    # the mask call's own refusals
    for mode in (2, 3):
        assert call([g0, None, (mode, box, pay[:900])]) == YK_ERR_BAD_ARG                              # no 'MIPM': w == 0
        assert call([g0, None, (mode, box, pay[:900], bits, grid)], null_bits=(2,)) == YK_ERR_BAD_ARG   # NULL bits
        assert call([g0, None, (mode, (20, 5, 42, 30), pay[:900], bits, grid)]) == YK_ERR_BAD_ARG       # width not a multiple of 4
    for bad_grid in ((0, 0, -1, 2), (0, 0, 3, -2), (0, 0, 4, 4), (0, 0, 16, 1)):                        # negative, or more than the 15 tiles of the image
        assert call([g0, None, (3, box, pay[:900], np.full(8, 0xFF, np.uint8), bad_grid)]) == YK_ERR_BAD_ARG, bad_grid
    assert call([g0, None, (3, box, pay[:900], bits, (0, 0, 5, 3))], mip_bytes={2: 1}) == YK_ERR_RANGE   # 15 tiles need 2 bytes
    assert "'MIPM' bitmap shorter" in lib().yk_last_error(dec._h).decode()
    nul = (C.c_size_t * n)(0, 0, 0)
    modes = np.full(n, -1, np.int32)
    assert L.yk_decode_alpha_mask_batch_device(dec._h, modes.ctypes.data, np.zeros((n, 4), np.int32).ctypes.data, (C.c_void_p * n)(), nul, None, None, None,
                                               255) == YK_ERR_BAD_ARG
    # the existing call keeps refusing the mask modes
    for mode in (2, 3):
        assert call([g0, None, (mode, box, pay[:900])], masks=False) == YK_ERR_BAD_ARG
        assert "mask modes" in lib().yk_last_error(dec._h).decode()
    dec.synchronize()
    for f in range(n):                                                       # the earlier planes are still there, untouched
        dec.select_frame(f)
        np.testing.assert_array_equal(dec.alpha_plane(), want[f], err_msg=f"frame {f}")
    assert dec.alpha_batch_status().tolist() == [0, 0, 0]
    assert call(good) == 0                                                   # and the handle still works
    # the single-image calls still refuse a batch
    box4 = (C.c_int32 * 4)(0, 0, 16, 16)
    out = np.zeros(3 * 2 * 32, np.uint8)
    assert L.yk_decode_mask(dec._h, bits.ctypes.data, 3, 2, out.ctypes.data, out.size) == YK_ERR_STATE
    assert L.yk_decode_alpha(dec._h, 6, box4, pay.ctypes.data, 256, None, 0, None, 0) == YK_ERR_STATE


def test_rgba_output_from_the_masked_planes(dec, dec1):
    """image_batch_device(channels=4, alpha_from_planes=True) after the masked call = the per-frame RGBA"""
    ent, w, h = _five_72x40(np.random.default_rng(46))
    dec.begin_batch(w, h, len(ent))                                          # no colour chunks: the planes are the cleared ones, the same in every frame
    dec.decompress_alpha_batch(ent, 201)
    got = dec.image_batch_device(channels=4, alpha_from_planes=True).cpu().numpy()
    rgb = dec.image_batch_device(channels=4, alpha=255).cpu().numpy()
    for f, e in enumerate(ent):
        np.testing.assert_array_equal(got[f, ..., :3], rgb[f, ..., :3], err_msg=f"frame {f}")
        np.testing.assert_array_equal(got[f, ..., 3], _want(e, w, h, 201), err_msg=f"frame {f}")
        dec.select_frame(f)
        np.testing.assert_array_equal(dec.image_device(channels=4, alpha=-1).cpu().numpy(), got[f], err_msg=f"frame {f}: per-frame RGBA")
