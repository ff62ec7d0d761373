"""The 6-bit mask mode of the 'ALPM' values for batches: yk_alpha_values_mask_batch (HipTileEncoder.alpha_values_mask_batch /
alpha_mask_payloads_device) and HipTileDecoder.decode_batch_from_encoder(alpha_6bit=True).  Every comparison is bit-exact, against two independent
sources: the numpy restatement of ProcessAlpha (tests/alpha_ref.py) with the tile rule's mask on the bounds the handle reports, and
yk_alpha_values(force8Bit) of a second handle on the frame alone.  The frames are those of tests/alpha6_cases.py; tests/test_alpha6_batch_layout.py
confirms on the CPU that they give the modes asserted here, a mode-3 frame with a rejected tile inside its box in every batch whose shape has room
for one (not 16 x 16) and a mode-3 frame whose kept tiles span the image wherever the sides are multiples of 16 (16 x 16, 80 x 48)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import alpha6_cases as A
from tests import alpha_ref as R
from tests.test_alpha_6bit_mask import tile_mask
from yaik_amd._lib import lib
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_STATE = -2, -4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Info(C.Structure):
    _fields_ = [("mode", C.c_int32), ("bbox", C.c_int32 * 4), ("rawSize", C.c_uint32)]


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def enc():
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def one():
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dec():
    d = HipTileDecoder(0)
    yield d
    d.close()


def _same(got, want, what):
    if want is None:
        assert got is None, (what, got)
        return
    assert got is not None, (what, want["mode"], want["bbox"])
    assert got["mode"] == want["mode"] and tuple(got["bbox"]) == tuple(int(v) for v in want["bbox"]), (what, got["mode"], got["bbox"], want["mode"], want["bbox"])
    np.testing.assert_array_equal(got["payload"], want["payload"], err_msg=str(what))


def _flag(force8bit, f):
    """frame f's force8Bit: None is 0 for every frame"""
    if force8bit is None or isinstance(force8bit, bool):
        return bool(force8bit)
    return bool(force8bit[f])


def _single(one, planes, f8, cache=None, key=None):
    """yk_alpha_values(f8) of the second handle on the frame alone: (bounds, result)"""
    if cache is not None and (key, f8) in cache:
        return cache[(key, f8)]
    one.set_image(planes)
    mp = one.mip_prefilter()
    out = (mp["bounds"], one.alpha_values(f8))
    if cache is not None:
        cache[(key, f8)] = out
    return out


def _bind(enc, frames, unaligned=False):
    torch = _torch()
    if not unaligned:
        t = torch.from_numpy(frames).cuda()
    else:                                                                   # the planes start 4 bytes behind a 16-byte boundary
        buf = torch.empty(frames.size + 1, dtype=torch.int32, device="cuda")
        t = buf[1:].view(frames.shape)
        t.copy_(torch.from_numpy(frames))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    enc.set_batch(t)
    enc.encode_batch()


def _check(enc, one, frames, force8bit=None, cache=None, what="", bound=False, masks=None):
    """alpha_values_mask_batch(force8bit) of the frames against both references; masks[f]: a per-pixel mask in place of the tile rule's"""
    n = frames.shape[0]
    if not bound:
        _bind(enc, frames)
    got = enc.alpha_values_mask_batch(force8bit)
    dev = enc.alpha_mask_payloads_device(force8bit)
    assert len(got) == n and len(dev) == n
    end = {}
    for f in range(n):
        f8 = _flag(force8bit, f)
        enc.select_frame(f)
        bounds = enc.alpha_result()["bounds"]
        if frames[f, 3].any():                                              # the model the CPU test checks the coverage with
            np.testing.assert_array_equal(bounds, A.model_bounds(frames[f, 3]), err_msg=f"{what} frame {f}")
        m = tile_mask(frames[f, 3], bounds) if masks is None else masks[f]
        _same(got[f], R.encode(frames[f, 3], bounds, m, f8), (what, f, "restatement"))
        b1, want1 = _single(one, frames[f], f8, cache, f)
        np.testing.assert_array_equal(b1, bounds)
        _same(got[f], want1, (what, f, "single handle"))
        if got[f] is None:
            assert dev[f] is None
            continue
        mode, bbox, ptr, nb = dev[f][:4]
        assert (mode, bbox, nb) == (got[f]["mode"], got[f]["bbox"], got[f]["payload"].size) and ptr % 16 == 0 and ptr
        end[ptr] = ptr + nb
    spans = sorted(end.items())                                             # no two payloads overlap
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    return got


# ---- 1. shapes, counts, kinds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", A.COUNTS)
@pytest.mark.parametrize("w,h", A.SHAPES)
def test_parity(enc, one, w, h, n):
    kinds, frames = A.frames_of(w, h, n)
    got = _check(enc, one, frames, None, {}, (w, h, n))
    assert [None if g is None else g["mode"] for g in got] == [A.KIND_MODE[k] for k in kinds]
    three = [f for f, g in enumerate(got) if g is not None and g["mode"] == 3]
    if (w, h) != (16, 16) and (n > 1 or (w, h) != (80, 48)):
        assert any(A.has_rejected_tile_in_box(frames[f, 3]) for f in three)
    if (w, h) in ((16, 16), (80, 48)):
        assert any(A.spans_image(frames[f, 3]) for f in three)
    if (w, h) == (1040, 40) and kinds[0] == "ring":
        assert got[0]["bbox"][0] == 0 and got[0]["bbox"][2] == 1040                     # 65 tile columns: the band kernel's carry
    for f, g in enumerate(got):                                             # 3/4 of the 8-bit payload, less what rejected tiles drop
        if g is not None and g["mode"] == 3:
            assert g["payload"].size <= g["bbox"][2] // 4 * 3 * g["bbox"][3]


# ---- 2. force8Bit per frame -------------------------------------------------------------------------------------------------------------------------
def test_mixed_force8bit(enc, one):
    w, h, n = 72, 40, 12
    kinds, frames = A.frames_of(w, h, n, seed=1)
    cache = {}
    alt = [f & 1 for f in range(n)]
    got = _check(enc, one, frames, alt, cache, "alternating")
    want_modes = [A.KIND_MODE[k] if not alt[f] else {3: 6}.get(A.KIND_MODE[k], A.KIND_MODE[k]) for f, k in enumerate(kinds)]
    assert [None if g is None else g["mode"] for g in got] == want_modes and 3 in want_modes and 6 in want_modes
    # all 1: yk_alpha_values_batch's infos, payloads and slots -- nothing of the 6-bit path is handed out.  That the three 6-bit launches, the
    # third read-back and the second upload are skipped (and the budget of six launches and three read-backs in general) is NOT observed here: the
    # project has no launch counter, so that rests on the code (`if (n6)` in yk_alpha_values_mask_batch; DESIGN 21 says the same)
    _bind(enc, frames)
    eight = enc.alpha_values_batch()
    eight_dev = enc.alpha_payloads_device()
    for flags in (True, [1] * n, np.ones(n, bool)):
        got = enc.alpha_values_mask_batch(flags)
        dev = enc.alpha_mask_payloads_device(flags)
        for f in range(n):
            _same(got[f], eight[f], ("all 1", f))
            assert (dev[f] is None and eight_dev[f] is None) or dev[f][:4] == eight_dev[f]
    assert not any(g is not None and g["mode"] == 3 for g in got)
    _check(enc, one, frames, None, cache, "NULL", bound=True)
    _check(enc, one, frames, False, cache, "False", bound=True)
    # no analog frame at all: binary, all-255 and empty only
    rng = np.random.default_rng(5)
    kinds = ["binary", "all255", "empty", "low13", "binary"]
    frames = np.stack([np.concatenate([A.rgb(h, w, f), A.alpha_of(rng, h, w, k)[None]]) for f, k in enumerate(kinds)])
    got = _check(enc, one, frames, None, {}, "no analog frame")
    assert [None if g is None else g["mode"] for g in got] == [1, None, None, None, 1]
    with pytest.raises(ValueError):
        enc.alpha_values_mask_batch([0, 1])


# ---- 3. the fixtures captured from the reference with force8Bit = 0 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["alpha_analog_6bit_mask.npz", "alpha_analog_6bit_fullmask.npz"])
def test_fixture(enc, one, name):
    """the shapes of the two fixtures differ (160 x 112, 64 x 80): each is a batch of one.  The comparison rule is
    test_gpu_encode_6bit_matches_fixture's: the captured mask inside the captured bounds, the tile rule outside them"""
    z = dict(np.load(os.path.join(GOLDEN, name)))
    a = z["alpha"].astype(np.int32)
    h, w = a.shape
    frames = np.concatenate([A.rgb(h, w, 0), a[None]])[None]
    mask = tile_mask(a, A.model_bounds(a))
    x0, y0, x1, y1 = (int(v) for v in z["bounds"])
    mask[y0:y1, x0:x1] = z["mipmask"][y0:y1, x0:x1] != 0
    got = _check(enc, one, frames, None, {}, name, masks=[mask])
    assert got[0]["mode"] == R.IS_6_BIT_USEMIPMAPMASK_INVERSE
    enc.select_frame(0)
    if np.array_equal(enc.alpha_result()["bounds"], z["bounds"]):          # the search region is the reference's: header and payload are too
        hd = z["header"]
        assert got[0]["bbox"] == tuple(int(v) for v in hd[:4]) and len(got[0]["payload"]) == hd[5]
        np.testing.assert_array_equal(got[0]["payload"], z["payload"])


# ---- 4. planes that are not 16-byte aligned -----------------------------------------------------------------------------------------------------------
def test_unaligned_planes(enc, one):
    """The handle binds no plane at a base that is not 16-byte aligned (yk_bind_device_planes / yk_bind_device_batch refuse it, as they always have;
    row and frame pitches are multiples of 4 samples), so the classify path's non-vector loads cannot be reached through the public calls.  What can
    be asked is asked: the bind is refused, and the batch bound before it gives the same payloads afterwards."""
    from yaik_amd._lib import YaikError
    _, frames = A.frames_of(72, 40, 7, seed=2)
    aligned = _check(enc, one, frames, None, {}, "aligned")
    fresh = HipTileEncoder(0)                                                # a handle reports the first failure it ever had: a new one
    try:
        with pytest.raises(YaikError, match="16-byte aligned"):
            _bind(fresh, frames, unaligned=True)
        got = _check(fresh, one, frames, None, None, "after the refused bind")
    finally:
        fresh.close()
    for f in range(len(got)):
        _same(got[f], aligned[f], f)


# ---- 5. handle state ------------------------------------------------------------------------------------------------------------------------------
def test_calls_in_a_row_on_one_handle(enc, one):
    _check(enc, one, A.frames_of(80, 48, 7, seed=3)[1], None, {}, "seven frames")
    _check(enc, one, A.frames_of(80, 48, 3, seed=4)[1], None, {}, "fewer frames")
    _, small = A.frames_of(72, 40, 3, seed=5)
    _check(enc, one, small, None, {}, "a smaller shape")
    eight = enc.alpha_values_batch()                                         # the 8-bit call in between
    for f in range(3):
        enc.select_frame(f)
        _same(eight[f], R.encode(small[f, 3], enc.alpha_result()["bounds"], None, True), ("8-bit", f))
    got = _check(enc, one, small, [0, 1, 0], {}, "again", bound=True)
    # yk_alpha_bitmaps_batch in between touches none of the payloads
    dev = enc.alpha_mask_payloads_device([0, 1, 0])
    enc.alpha_bitmaps_batch()
    L = lib()
    for f, g in enumerate(got):
        if g is None:
            continue
        pay, nb = np.zeros(g["payload"].size, np.uint8), C.c_size_t()
        assert L.yk_alpha_payload(enc._h, f, pay.ctypes.data, pay.size, C.byref(nb)) == 0 and nb.value == pay.size
        np.testing.assert_array_equal(pay, g["payload"])
        assert dev[f][:2] == (g["mode"], g["bbox"])
    with_bits = enc.alpha_mask_payloads_device([0, 1, 0])                      # the bits of alpha_bitmaps_batch ride along
    mips = enc.alpha_bitmaps_device()
    for f, e in enumerate(with_bits):
        if e is not None:
            assert e[4:6] == (mips[f]["ptr"], mips[f]["nbytes"]) and (e[6] == tuple(int(v) for v in mips[f]["tile_bbox"]) or not e[5])


def test_single_image_call_unpublishes_the_slots(enc):
    L = lib()
    _, frames = A.frames_of(80, 48, 1, first=0)
    if enc.frames != 1:                                                     # yk_set_image keeps the frame count of a batch of the same shape
        assert L.yk_set_batch(enc._h, 1) == 0
    enc.set_image(frames[0])
    mp = enc.mip_prefilter()
    got = enc.alpha_values_mask_batch()                                      # a batch of one behind yk_alpha_reject + yk_alpha_finish
    assert len(got) == 1
    _same(got[0], A.want(frames[0, 3], mp["bounds"], False), "batch of one")
    dev, nb = C.c_void_p(), C.c_size_t()
    assert L.yk_alpha_payload_device(enc._h, 0, C.byref(dev), C.byref(nb)) == 0 and dev.value and nb.value == got[0]["payload"].size
    _same(enc.alpha_values(False), got[0], "single call")
    assert L.yk_alpha_payload_device(enc._h, 0, C.byref(dev), C.byref(nb)) == YK_ERR_STATE and dev.value is None and nb.value == 0
    _same(enc.alpha_values_mask_batch()[0], got[0], "and published again")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
def _refused(h, rc, code, word):
    assert rc == code, (rc, code, word)
    msg = lib().yk_last_error(h).decode()
    assert word in msg, (word, msg)


def test_refusals(enc, one):
    """NULL infos, before the alpha stage, on a stripe.  The two remaining refusals (no planes bound, no keep flags) guard states that no sequence
    of public calls reaches once the alpha stage has finished: they are not provoked here."""
    torch = _torch()
    L = lib()
    w, h, n = 80, 48, 3
    kinds, frames = A.frames_of(w, h, n, seed=6)
    infos = (Info * n)()
    _bind(enc, frames)
    good = enc.alpha_values_mask_batch()
    dev0, nb0 = C.c_void_p(), C.c_size_t()
    assert L.yk_alpha_payload_device(enc._h, 0, C.byref(dev0), C.byref(nb0)) == 0 and dev0.value
    _refused(enc._h, L.yk_alpha_values_mask_batch(enc._h, None, None), YK_ERR_BAD_ARG, "infos")
    dev, nb = C.c_void_p(), C.c_size_t()                                     # the earlier payloads are still published
    assert L.yk_alpha_payload_device(enc._h, 0, C.byref(dev), C.byref(nb)) == 0 and (dev.value, nb.value) == (dev0.value, nb0.value)
    pay = np.zeros(nb.value, np.uint8)
    assert L.yk_alpha_payload(enc._h, 0, pay.ctypes.data, pay.size, C.byref(nb)) == 0
    np.testing.assert_array_equal(pay, good[0]["payload"])
    _refused(enc._h, L.yk_alpha_values_batch(enc._h, 0, infos), YK_ERR_BAD_ARG, "6-bit mask mode")      # pinned: the 8-bit call refuses as before
    enc.set_batch(torch.from_numpy(frames).cuda())                           # bound, the alpha stage has not run
    _refused(enc._h, L.yk_alpha_values_mask_batch(enc._h, None, infos), YK_ERR_STATE, "alpha stage")
    planes = np.concatenate([frames[0], frames[1], frames[2][:, :33]], axis=1)                        # 129 rows: 128 owned + 1 halo of a 192-row image
    enc.set_image(planes, full_h=192, y0=0, halo_rows=1)
    enc.alpha_reject()
    enc.alpha_finish(np.array([0, 0, w, 192], np.int32))
    _refused(enc._h, L.yk_alpha_values_mask_batch(enc._h, None, infos), YK_ERR_STATE, "stripe")
    got = _check(enc, one, frames, None, {}, "after the refusals")            # the handle works afterwards
    assert [None if g is None else g["mode"] for g in got] == [A.KIND_MODE[k] for k in kinds]
    enc.set_batch(torch.from_numpy(np.ascontiguousarray(frames[:, :3])).cuda())          # RGB: no alpha plane, nothing launched
    enc.encode_batch()
    assert enc.alpha_values_mask_batch() == [None] * n and enc.alpha_mask_payloads_device([1, 0, 1]) == [None] * n


# ---- 7. round trip on the device ------------------------------------------------------------------------------------------------------------------
def _decodable_frames(w, h):
    """analog frames whose box of kept tiles is not the image and has every tile kept (the decodable rule), a binary frame, a frame without a chunk"""
    rng = np.random.default_rng(77)
    boxes = [(16, 16, 64, 48), (0, 0, 48, 32), (32, 16, 80, 32), (16, 0, 32, 48)]
    alphas = []
    for x0, y0, x1, y1 in boxes:
        a = np.zeros((h, w), np.int32)
        a[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0))
        for ty in range(y0, y1, 16):                                         # every tile of the box holds a sample
            for tx in range(x0, x1, 16):
                a[ty + int(rng.integers(0, 16)), tx + int(rng.integers(0, 16))] = int(rng.integers(4, 256))
        alphas.append(a)
    alphas += [A.alpha_of(rng, h, w, "binary"), A.alpha_of(rng, h, w, "all255")]
    return np.stack([np.concatenate([A.rgb(h, w, f), a[None]]) for f, a in enumerate(alphas)])


def test_round_trip_on_the_device(enc, dec):
    from yaik_amd.files import alpha6_decodable
    w, h = 80, 48
    frames = _decodable_frames(w, h)
    n = frames.shape[0]
    _bind(enc, frames)
    mips = enc.alpha_bitmaps_batch()
    assert [alpha6_decodable(m["has_chunk"], m["tile_bbox"], m["bitmap"]) for m in mips[:4]] == [True] * 4
    dec.begin_batch(w, h, n)
    dec.decode_batch_from_encoder(enc, alpha=True, alpha_6bit=True)
    got = dec.image_batch_device(channels=4, alpha_from_planes=True).cpu().numpy()
    assert dec.alpha_batch_status().tolist() == [0] * n
    sent = enc.alpha_values_mask_batch([m["bitmap"].size == 0 for m in mips])
    assert [None if e is None else e["mode"] for e in sent] == [3, 3, 3, 3, 1, None]
    for f in range(4):
        x, y, bw, bh = sent[f]["bbox"]
        v = frames[f, 3, y:y + bh, x:x + bw]
        want = np.zeros((h, w), np.uint8)
        want[y:y + bh, x:x + bw] = ((v >> 2) << 2) | (v >> 6)
        np.testing.assert_array_equal(got[f, ..., 3], want, err_msg=f"frame {f}")
    e = sent[4]
    np.testing.assert_array_equal(got[4, ..., 3], R.decode(e["mode"], e["bbox"], e["payload"], w, h, reference_1bit=False))
    assert bool((got[5, ..., 3] == 255).all())                               # no chunk: opaque
    eight = HipTileDecoder(0)                                                # the default keeps today's path, and the colours are the same
    try:
        eight.begin_batch(w, h, n)
        eight.decode_batch_from_encoder(enc, alpha=True)
        ref = eight.image_batch_device(channels=4, alpha_from_planes=True).cpu().numpy()
    finally:
        eight.close()
    np.testing.assert_array_equal(got[..., :3], ref[..., :3])
    for f in range(4):
        x, y, bw, bh = sent[f]["bbox"]
        np.testing.assert_array_equal(ref[f, y:y + bh, x:x + bw, 3], frames[f, 3, y:y + bh, x:x + bw].astype(np.uint8))
