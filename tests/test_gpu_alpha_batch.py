"""'ALPM' alpha values for batches: yk_alpha_values_batch + the payload getters, yk_decode_alpha_batch_device and
yk_decode_output_batch_alpha_device (HipTileEncoder.alpha_values_batch / alpha_payloads_device, HipTileDecoder.decompress_alpha_batch /
image_batch_device(alpha_from_planes=True) / decode_batch_from_encoder(alpha=True)).  Every comparison is bit-exact, against two independent
sources: the numpy restatement of the coder (tests/alpha_ref.py) and a second handle that runs the single-image calls on the same frame."""
import ctypes as C

import numpy as np
import pytest

from tests import alpha_ref as R
from yaik_amd._lib import YaikError, lib
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_ERR_RANGE = -2, -4, -5
SENTINEL = 0xA5
# 16 x 16: one tile; 72 x 40: width 8 mod 16; 1040 x 520: a box row wider than the 1024 pixels of one workgroup (blockIdx.x > 0)
SHAPES = [(16, 16), (72, 40), (80, 48), (1040, 520)]
COUNTS = [1, 2, 7, 33]
KINDS = ["analog", "binary", "all255", "low", "low_edges", "zero", "edges", "corners"]


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


@pytest.fixture(scope="module")
def dec1():
    d = HipTileDecoder(0)
    yield d
    d.close()


def _alpha(rng, h, w, kind, small=False):
    """one alpha plane (int32, 0..255) of the named class; small: the box stays inside the top-left quarter"""
    a = np.zeros((h, w), np.int32)
    hh, ww = (max(h // 2, 2), max(w // 2, 2)) if small else (h, w)
    y0, x0 = int(rng.integers(0, hh - 1)), int(rng.integers(0, ww - 1))
    y1, x1 = int(rng.integers(y0 + 1, hh + 1)), int(rng.integers(x0 + 1, ww + 1))
    if kind == "analog":
        a[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0))
        a[y0, x0] = a[y1 - 1, x1 - 1] = 77
    elif kind == "binary":
        a[y0:y1, x0:x1] = 255 * rng.integers(0, 2, (y1 - y0, x1 - x0))
        a[y0, x0] = a[y1 - 1, x1 - 1] = 255
    elif kind == "all255":
        a[:] = 255
    elif kind == "low":                                    # values 0..3 only: v >> 2 == 0 everywhere, an empty box
        a[y0:y1, x0:x1] = rng.integers(0, 4, (y1 - y0, x1 - x0))
    elif kind == "low_edges":                              # the pattern of test_gpu_alpha_values.py: one 255 among values 1..3
        a[y0:y1, x0:x1] = rng.integers(1, 4, (y1 - y0, x1 - x0))
        a[(y0 + y1) // 2, (x0 + x1) // 2] = 255
    elif kind == "edges":                                  # a box touching all four image edges
        a[:] = 255 * rng.integers(0, 2, (h, w))
        a[0, w // 2] = a[h - 1, w // 3] = a[h // 2, 0] = a[h // 3, w - 1] = 255
    elif kind == "corners":                                # a single pixel >= 4 in each corner
        a[0, 0], a[0, w - 1], a[h - 1, 0], a[h - 1, w - 1] = 4, 255, 9, 200
    elif kind != "zero":
        raise ValueError(kind)
    return a


def _rgb(h, w, f):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([((x * (p + 1) + y * 2 + 17 * p + 5 * f) & 255).astype(np.int32) for p in range(3)])


def _frames(w, h, n, first=0, seed=0, small=False):
    """n frames [n, 4, h, w] int32, frame f of class KINDS[(first + f) % 8]"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h * 3 + n)
    return np.stack([np.concatenate([_rgb(h, w, f), _alpha(rng, h, w, KINDS[(first + f) % len(KINDS)], small)[None]]) for f in range(n)])


def _same(got, want, what):
    if want is None:
        assert got is None, (what, got)
        return
    assert got is not None, (what, want["mode"], want["bbox"])
    assert got["mode"] == want["mode"] and tuple(got["bbox"]) == tuple(want["bbox"]), (what, got["mode"], got["bbox"], want["mode"], want["bbox"])
    np.testing.assert_array_equal(got["payload"], want["payload"], err_msg=str(what))


def _single(one, planes):
    """today's single-image path on a second handle: (bounds, alpha_values(True))"""
    one.set_image(planes)
    mp = one.mip_prefilter()
    return mp["bounds"], one.alpha_values(True)


def _check_batch(enc, one, frames, bind, ref=None):
    """ref: a dict that keeps the two references of these frames (computed once) for a second run with another way of binding"""
    torch = _torch()
    ref = {} if ref is None else ref
    n, _, h, w = frames.shape
    if bind == "planes":
        enc.set_batch(torch.from_numpy(frames).cuda())
    else:
        enc.set_batch_u8(torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 2, 3, 1)).astype(np.uint8)).cuda())
    enc.encode_batch()
    got = enc.alpha_values_batch()
    dev = enc.alpha_payloads_device()
    enc.synchronize()
    assert len(got) == n and len(dev) == n
    for f in range(n):
        enc.select_frame(f)
        bounds = enc.alpha_result()["bounds"]
        if f not in ref:
            ref[f] = _single(one, frames[f]) + (R.encode(frames[f, 3], bounds, None, True),)
        b1, want1, want2 = ref[f]
        _same(got[f], want2, (bind, f, "restatement"))
        assert np.array_equal(b1, bounds), (bind, f)
        _same(got[f], want1, (bind, f, "single handle"))
        if got[f] is None:
            assert dev[f] is None
        else:
            assert dev[f][:2] == (got[f]["mode"], got[f]["bbox"]) and dev[f][3] == got[f]["payload"].size and dev[f][2] % 16 == 0
    return got


# ---- 1. encode parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_encode_parity(enc, one, w, h, n):
    frames = _frames(w, h, n, first=SHAPES.index((w, h)) * 3 + n)          # every class comes first in some small batch
    ref = {}
    got = _check_batch(enc, one, frames, "planes", ref)
    again = _check_batch(enc, one, frames, "u8", ref)
    for f in range(n):
        _same(again[f], got[f], f)
    if n >= len(KINDS):                                                     # the classes are what their names say
        modes = {KINDS[(SHAPES.index((w, h)) * 3 + n + f) % len(KINDS)]: (g["mode"] if g else None) for f, g in enumerate(got)}
        assert modes["analog"] == 6 and modes["binary"] == 1 and modes["edges"] == 1 and modes["corners"] == 6
        assert modes["all255"] is None and modes["low"] is None and modes["zero"] is None


def test_encode_without_alpha_plane(enc):
    torch = _torch()
    enc.set_batch(torch.from_numpy(np.ascontiguousarray(_frames(80, 48, 3)[:, :3])).cuda())
    enc.encode_batch()
    assert enc.alpha_values_batch() == [None, None, None] and enc.alpha_payloads_device() == [None, None, None]


def test_batch_of_one_after_mip_prefilter(enc, one):
    """a batch of one takes the same path behind yk_alpha_reject + yk_alpha_finish"""
    frames = _frames(80, 48, 2, first=0)
    for f in range(2):
        enc.set_image(frames[f])
        mp = enc.mip_prefilter()
        got = enc.alpha_values_batch()
        assert len(got) == 1
        _same(got[0], R.encode(frames[f, 3], mp["bounds"], None, True), f)
        _same(got[0], enc.alpha_values(True), f)


# ---- 2. stale state -----------------------------------------------------------------------------------------------------------------------------
def test_second_batch_sees_nothing_of_the_first(enc, one):
    w, h = 80, 48
    _check_batch(enc, one, _frames(w, h, 7, first=0, seed=1), "planes")
    _check_batch(enc, one, _frames(w, h, 3, first=0, seed=2), "planes")                 # fewer frames
    _check_batch(enc, one, _frames(w, h, 3, first=0, seed=3, small=True), "planes")     # then smaller boxes
    _check_batch(enc, one, _frames(w, h, 3, first=5, seed=4, small=True), "u8")         # then other classes in the same slots


# ---- 3. decode parity ---------------------------------------------------------------------------------------------------------------------------
def _entry(rng, w, h, mode):
    step = 8 if mode == R.IS_1_BIT_FULL else 4 if mode in (R.IS_6_BIT_FULL, R.IS_6_BIT_FULL_INVERSE) else 1
    bw = int(rng.integers(1, w // step + 1)) * step
    bh = int(rng.integers(1, h + 1))
    bx = int(rng.integers(0, (w - bw) // step + 1)) * step
    by = int(rng.integers(0, h - bh + 1))
    n = {R.IS_8_BIT_FULL: bw * bh, R.IS_1_BIT_FULL: bw // 8 * bh}.get(mode, bw // 4 * 3 * bh)
    return (mode, (bx, by, bw, bh), rng.integers(0, 256, n + int(rng.integers(0, 5)), dtype=np.uint8))   # up to 4 spare bytes behind the payload


def _entries(w, h, seed):
    rng = np.random.default_rng(seed + w * 13 + h)
    order = [R.IS_8_BIT_FULL, None, R.IS_1_BIT_FULL, R.IS_6_BIT_FULL, R.IS_6_BIT_FULL_INVERSE, None, R.IS_1_BIT_FULL, R.IS_8_BIT_FULL, R.IS_6_BIT_FULL]
    ent = [None if m is None else _entry(rng, w, h, m) for m in order]
    ent.append((R.IS_8_BIT_FULL, (0, 0, w, h), rng.integers(0, 256, w * h, dtype=np.uint8)))          # a box that is the whole image
    return ent


def _want_plane(e, w, h, fill):
    return np.full((h, w), fill, np.uint8) if e is None else R.decode(e[0], e[1], e[2], w, h, reference_1bit=False)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_decode_parity(dec, dec1, w, h, where):
    torch = _torch()
    ent = _entries(w, h, 31)
    fill = 255 if where == "host" else 93
    dec.begin_batch(w, h, len(ent))
    if where == "host":
        dec.decompress_alpha_batch(ent, fill)
    else:
        keep = [None if e is None else torch.from_numpy(e[2]).cuda() for e in ent]
        torch.cuda.synchronize()
        dec.decompress_alpha_batch([None if e is None else (e[0], e[1], t.data_ptr(), e[2].size) for e, t in zip(ent, keep)], fill)
    for f, e in enumerate(ent):
        dec.select_frame(f)
        got = dec.alpha_plane()
        np.testing.assert_array_equal(got, _want_plane(e, w, h, fill), err_msg=f"frame {f}")
        if e is not None:                                                   # the same entry on a single-image decoder
            dec1.begin(w, h)
            np.testing.assert_array_equal(got, dec1.decompress_alpha(e[0], e[1], e[2]), err_msg=f"frame {f}")
    dec.begin_batch(w, h, len(ent))                                         # a new batch has no planes
    with pytest.raises(YaikError):
        dec.alpha_plane()


# ---- 4. output ----------------------------------------------------------------------------------------------------------------------------------
def _decoded_batch(enc, dec, w, h, n, seed):
    """a batch with real colour planes (from a batch encode of RGB frames) and random alpha entries"""
    torch = _torch()
    enc.set_batch(torch.from_numpy(np.ascontiguousarray(_frames(w, h, n, seed=seed)[:, :3])).cuda())
    enc.encode_batch()
    dec.begin_batch(w, h, n)
    dec.decode_batch_from_encoder(enc)
    ent = _entries(w, h, seed)[:n]
    dec.decompress_alpha_batch(ent, 201)
    return ent


@pytest.mark.parametrize("planar", [False, True], ids=["hwc", "chw"])
@pytest.mark.parametrize("w,h", [(80, 48), (72, 40)])
def test_output_layouts(enc, dec, w, h, planar):
    torch = _torch()
    n = 4
    ent = _decoded_batch(enc, dec, w, h, n, 5)
    planes = [_want_plane(e, w, h, 201) for e in ent]
    const = dec.image_batch_device(channels=4, alpha=17, planar=planar).cpu().numpy()
    tight = dec.image_batch_device(channels=4, planar=planar, alpha_from_planes=True).cpu().numpy()
    want = const.copy()
    for f in range(n):
        if planar:
            want[f, 3] = planes[f]
        else:
            want[f, ..., 3] = planes[f]
    assert not np.array_equal(want, const)
    np.testing.assert_array_equal(tight, want)                              # alpha = the plane, RGB = the constant-alpha output
    for f in range(n):                                                      # each frame = select_frame + image_device(alpha=-1)
        dec.select_frame(f)
        np.testing.assert_array_equal(dec.image_device(channels=4, alpha=-1, planar=planar).cpu().numpy(), want[f])
    for off in (1, 2, 3):                                                   # padded row, plane and frame pitches at a base offset
        row = (w if planar else 4 * w) + 5 + off
        plane = row * h + 11
        frame = (4 * plane if planar else row * h) + 23
        buf = torch.full((off + n * frame + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(buf, (n, 4, h, w), (frame, plane, row, 1), off) if planar else torch.as_strided(buf, (n, h, w, 4), (frame, row, 4, 1), off)
        dec.image_batch_device(out=view, channels=4, planar=planar, alpha_from_planes=True)
        dec.synchronize()
        exp = np.full(buf.numel(), SENTINEL, np.uint8)
        ev = np.lib.stride_tricks.as_strided(exp[off:], (n, 4, h, w), (frame, plane, row, 1)) if planar else \
            np.lib.stride_tricks.as_strided(exp[off:], (n, h, w, 4), (frame, row, 4, 1))
        ev[...] = want
        np.testing.assert_array_equal(buf.cpu().numpy(), exp, err_msg=f"offset {off}")


# ---- 5. round trip from the encoder ---------------------------------------------------------------------------------------------------------------
def test_round_trip_from_encoder(enc, dec, dec1):
    torch = _torch()
    w, h, n = 80, 48, 7
    frames = _frames(w, h, n, first=0, seed=9)
    px = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 2, 3, 1)).astype(np.uint8)).cuda()
    enc.set_batch_u8(px)
    enc.encode_batch()
    dec.begin_batch(w, h, n)
    dec.decode_batch_from_encoder(enc, alpha=True)
    got = dec.image_batch_device(channels=4, alpha_from_planes=True).cpu().numpy()
    dec1.begin_batch(w, h, n)
    dec1.decode_batch_from_encoder(enc)                                     # alpha=False: today's behaviour
    rgb = dec1.image_batch_device(channels=4, alpha=255).cpu().numpy()
    np.testing.assert_array_equal(got[..., :3], rgb[..., :3])
    chunks = 0
    for f in range(n):
        enc.select_frame(f)
        e = R.encode(frames[f, 3], enc.alpha_result()["bounds"], None, True)
        want = np.full((h, w), 255, np.uint8) if e is None else R.decode(e["mode"], e["bbox"], e["payload"], w, h, reference_1bit=False)
        chunks += e is not None
        np.testing.assert_array_equal(got[f, ..., 3], want, err_msg=f"frame {f} ({KINDS[f]})")
        if e is not None and e["mode"] == R.IS_8_BIT_FULL:                   # 8-bit alpha comes back exactly inside its box
            x, y, bw, bh = e["bbox"]
            np.testing.assert_array_equal(got[f, y:y + bh, x:x + bw, 3], frames[f, 3, y:y + bh, x:x + bw].astype(np.uint8))
    assert 3 <= chunks < n


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
def _refused(h, rc, code, word):
    assert rc == code, (rc, code, word)
    msg = lib().yk_last_error(h).decode()
    assert word in msg, (word, msg)


def test_encode_refusals(enc, one):
    torch = _torch()
    L = lib()

    class Info(C.Structure):
        _fields_ = [("mode", C.c_int32), ("bbox", C.c_int32 * 4), ("rawSize", C.c_uint32)]

    w, h, n = 80, 48, 3
    frames = _frames(w, h, n, first=0, seed=11)                             # analog, binary, all255
    infos = (Info * n)()
    dev, nb = C.c_void_p(), C.c_size_t()
    enc.set_batch(torch.from_numpy(frames).cuda())
    _refused(enc._h, L.yk_alpha_values_batch(enc._h, 1, infos), YK_ERR_STATE, "alpha stage")          # before the alpha stage has run
    _refused(enc._h, L.yk_alpha_payload_device(enc._h, 0, C.byref(dev), C.byref(nb)), YK_ERR_STATE, "yk_alpha_values_batch first")
    enc.encode_batch()
    _refused(enc._h, L.yk_alpha_payload_device(enc._h, 0, C.byref(dev), C.byref(nb)), YK_ERR_STATE, "yk_alpha_values_batch first")
    _refused(enc._h, L.yk_alpha_values_batch(enc._h, 1, None), YK_ERR_BAD_ARG, "infos")
    _refused(enc._h, L.yk_alpha_values_batch(enc._h, 0, infos), YK_ERR_BAD_ARG, "6-bit mask mode")
    fresh = HipTileEncoder(0)                                                # pinned: the single-image call refuses a batch as before
    try:
        fresh.set_batch(torch.from_numpy(frames).cuda())
        fresh.encode_batch()
        with pytest.raises(YaikError, match="single image"):
            fresh.alpha_values(True)
    finally:
        fresh.close()
    with pytest.raises(YaikError):
        enc.alpha_values(True)
    got = enc.alpha_values_batch()                                           # the handle still works
    for f in range(n):
        enc.select_frame(f)
        _same(got[f], R.encode(frames[f, 3], enc.alpha_result()["bounds"], None, True), f)
    assert got[0]["mode"] == 6 and got[1]["mode"] == 1 and got[2] is None
    for f in (-1, n):
        _refused(enc._h, L.yk_alpha_payload_device(enc._h, f, C.byref(dev), C.byref(nb)), YK_ERR_BAD_ARG, "frame out of range")
        assert dev.value is None and nb.value == 0
    assert L.yk_alpha_payload_device(enc._h, 2, C.byref(dev), C.byref(nb)) == 0 and dev.value is None and nb.value == 0   # no chunk
    size = got[0]["payload"].size
    buf = np.full(size + 8, SENTINEL, np.uint8)
    _refused(enc._h, L.yk_alpha_payload(enc._h, 0, buf.ctypes.data, size - 1, C.byref(nb)), YK_ERR_RANGE, "too small")
    assert nb.value == size and np.all(buf == SENTINEL)
    assert L.yk_alpha_payload(enc._h, 0, buf.ctypes.data, size, C.byref(nb)) == 0 and nb.value == size
    assert np.array_equal(buf[:size], got[0]["payload"]) and np.all(buf[size:] == SENTINEL)
    # a stripe: the alpha values need the whole image
    planes = np.concatenate([frames[0], frames[1], frames[2][:, :33]], axis=1)                        # 129 rows: 128 owned + 1 halo of a 192-row image
    enc.set_image(planes, full_h=192, y0=0, halo_rows=1)
    enc.alpha_reject()
    enc.alpha_finish(np.array([0, 0, w, 192], np.int32))
    _refused(enc._h, L.yk_alpha_values_batch(enc._h, 1, infos), YK_ERR_STATE, "stripe")
    _check_batch(enc, one, frames, "planes")                                 # and still works afterwards


def test_decode_refusals(enc, dec):
    torch = _torch()
    L = lib()
    w, h, n = 64, 48, 3
    pay = np.arange(w * h, dtype=np.uint32).astype(np.uint8)
    good = [(R.IS_8_BIT_FULL, (8, 4, 40, 30), pay[:1200]), None, (R.IS_1_BIT_FULL, (0, 0, 64, 48), pay[:384])]
    fresh = HipTileDecoder(0)
    try:                                                                     # before any begin
        with pytest.raises(YaikError, match="begin"):
            fresh.frames = n
            fresh.decompress_alpha_batch(good)
    finally:
        fresh.close()
    dec.begin_batch(w, h, n)
    out = torch.full((n, h, w, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(YaikError, match="alpha planes"):                     # no planes yet
        dec.image_batch_device(out=out, channels=4, alpha_from_planes=True)
    with pytest.raises(YaikError):                                           # and no plane for the single-image forms either
        dec.image_device(channels=4, alpha=-1)
    dec.decompress_alpha_batch(good, 255)
    want = [_want_plane(e, w, h, 255) for e in good]

    def bad(entries, code, word, fill=255):
        from yaik_amd.decoder import pack_alpha_batch
        pk = pack_alpha_batch(entries)
        stage = torch.from_numpy(pk.staging if pk.staging.size else np.zeros(16, np.uint8)).cuda()
        torch.cuda.synchronize()
        ptrs = (C.c_void_p * n)(*[None if x is None or (x[0] == "d" and not x[1]) else (stage.data_ptr() + x[1] if x[0] == "h" else x[1]) for x in pk.where])
        sizes = (C.c_size_t * n)(*[int(v) for v in pk.nbytes])
        _refused(dec._h, L.yk_decode_alpha_batch_device(dec._h, pk.modes.ctypes.data, pk.bboxes.ctypes.data, ptrs, sizes, fill), code, word)

    g0, g2 = good[0], good[2]
    for box in ((60, 0, 8, 8), (0, 44, 8, 8), (-8, 0, 8, 8), (0, 0, 0, 4), (0, 0, 8, 0), (64, 0, 8, 8)):
        bad([g0, None, (R.IS_8_BIT_FULL, box, pay)], YK_ERR_BAD_ARG, "outside the image")
    bad([g0, None, (R.IS_1_BIT_FULL, (0, 0, 12, 4), pay)], YK_ERR_BAD_ARG, "multiple of 8")
    bad([g0, (R.IS_6_BIT_FULL, (0, 0, 10, 4), pay), g2], YK_ERR_BAD_ARG, "multiple of 4")
    bad([(R.IS_6_BIT_FULL_INVERSE, (0, 0, 6, 4), pay), None, g2], YK_ERR_BAD_ARG, "multiple of 4")
    for m in (0, 7, 8):
        bad([g0, None, (m, (0, 0, 16, 16), pay)], YK_ERR_BAD_ARG, "not decodable")
    for m in (2, 3):
        bad([g0, None, (m, (0, 0, 16, 16), pay)], YK_ERR_BAD_ARG, "mask modes")
    bad([g0, None, (R.IS_8_BIT_FULL, (0, 0, 16, 16), 0, 256)], YK_ERR_BAD_ARG, "NULL alpha payload")
    bad(good, YK_ERR_BAD_ARG, "noChunkAlpha", fill=256)
    bad(good, YK_ERR_BAD_ARG, "noChunkAlpha", fill=-1)
    bad([g0, None, (R.IS_8_BIT_FULL, (0, 0, 16, 16), pay[:255])], YK_ERR_RANGE, "shorter")
    bad([g0, None, (R.IS_1_BIT_FULL, (0, 0, 16, 16), pay[:31])], YK_ERR_RANGE, "shorter")
    bad([(R.IS_6_BIT_FULL, (0, 0, 16, 16), pay[:191]), None, g2], YK_ERR_RANGE, "shorter")
    sizes = (C.c_size_t * n)(0, 0, 0)
    _refused(dec._h, L.yk_decode_alpha_batch_device(dec._h, None, None, None, sizes, 255), YK_ERR_BAD_ARG, "NULL table")
    with pytest.raises(ValueError):                                          # the Python layer: one entry per frame
        dec.decompress_alpha_batch(good[:2])
    for f in range(n):                                                       # the earlier planes are still there, untouched
        dec.select_frame(f)
        np.testing.assert_array_equal(dec.alpha_plane(), want[f])
    # the output entry: layout refusals write nothing
    for args in ((None, 4 * w, 0, 4 * w * h), (out.data_ptr(), 4 * w - 1, 0, 4 * w * h), (out.data_ptr(), 4 * w, 0, 4 * w * h - 1),
                 (out.data_ptr(), w - 1, w * h, 4 * w * h), (out.data_ptr(), w, w * h - 1, 4 * w * h), (out.data_ptr(), w, w * h, 4 * w * h - 1)):
        assert L.yk_decode_output_batch_alpha_device(dec._h, *args) == YK_ERR_BAD_ARG, args
    with pytest.raises(ValueError):
        dec.image_batch_device(channels=3, alpha_from_planes=True)
    dec.synchronize()
    assert bool((out == SENTINEL).all())
    # the pinned behaviours of the existing entry points
    box = (C.c_int32 * 4)(0, 0, 16, 16)
    _refused(dec._h, L.yk_decode_alpha(dec._h, 6, box, pay.ctypes.data, 256, None, 0, None, 0), YK_ERR_STATE, "not supported in a batch")
    _refused(dec._h, L.yk_decode_output_batch_device(dec._h, out.data_ptr(), 4 * w, 0, 4 * w * h, 4, -1), YK_ERR_BAD_ARG, "alpha must be 0..255")
    dec.synchronize()
    assert bool((out == SENTINEL).all())
    dec.image_batch_device(out=out, channels=4, alpha_from_planes=True)     # the handle still works
    got = out.cpu().numpy()
    for f in range(n):
        np.testing.assert_array_equal(got[f, ..., 3], want[f])
    dec.begin_batch(w, h, n)                                                 # begin invalidates the planes
    with pytest.raises(YaikError, match="alpha planes"):
        dec.image_batch_device(out=out, channels=4, alpha_from_planes=True)
    dec.begin(w, h)                                                          # a single image: yk_decode_alpha as before, a batch of one on top
    one_plane = dec.decompress_alpha(*good[0])
    np.testing.assert_array_equal(one_plane, want[0])
    dec.begin(w, h)
    with pytest.raises(YaikError):
        dec.alpha_plane()
