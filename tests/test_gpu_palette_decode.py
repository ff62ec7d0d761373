"""PaletteDecompressor on the GPU (yk_palette_decompress_streams; HipTileDecoder.palette_*): every output byte for byte against the CPU oracle's
decode of the SAME payload (pyoracle.palette_decompress), and zero / non-zero status against the oracle's accept / reject.  The payloads and what
the oracle alone does with them are in tests/palette_payloads.py and tests/test_palette_decode_layout.py."""
import ctypes as C

import numpy as np
import pytest

from tests import palette_payloads as PP
from tests import palette_streams as PS
from tests.images import edge_image, synth_planes
from yaik_amd._lib import YaikError
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_ERR_RANGE = -2, -4, -5
YK_STAGE_PALETTE_DEC = 10
CASES = PS.cases()
CORPUS = PP.corpus()


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def enc():
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected(oracle_built):
    """the oracle's verdict on every corpus item at remap 250, computed once"""
    return {it.name: PP.oracle_decode(it.payload, it.out_bytes, 250) for it in CORPUS}


def _dev(arrays):
    t = _torch()
    return [t.from_numpy(np.ascontiguousarray(a).copy()).cuda() if a.size else t.empty(0, dtype=t.uint8, device="cuda") for a in arrays]


def _same(got, want, what):
    assert got.size == want.size, (what, "length", got.size, want.size)
    if not np.array_equal(got, want):
        first = int(np.argmax(got != want))
        raise AssertionError((what, "first difference at byte", first, got[max(0, first - 6):first + 9].tolist(), want[max(0, first - 6):first + 9].tolist()))


def _run(d, payloads, out_bytes, remap=250):
    n = d.palette_decompress_streams(_dev(payloads), out_bytes, remap)
    assert n == len(payloads)
    return d.palette_status(), [d.palette_decoded(i) for i in range(n)]


def _check(d, payloads, out_bytes, want, what, remap=250):
    """want[i] = (accepted, bytes) by the oracle"""
    st, got = _run(d, payloads, out_bytes, remap)
    assert st.size == len(payloads)
    for i, (ok, w) in enumerate(want):
        assert (st[i] == 0) == ok, (what, i, "status", int(st[i]), "oracle accepts" if ok else "oracle rejects")
        assert got[i].size == out_bytes[i], (what, i)
        if ok and out_bytes[i]:
            _same(got[i], w, (what, i))
    return st, got


# ---- 1. the compressor's payloads, the six whose decode is not their stream included -------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_compressor_payloads_decode_like_the_oracle(dec, oracle_built, name):
    _, streams, chain = next(c for c in CASES if c[0] == name)
    pays = PS.oracle_payloads(streams, chain)
    outs = [int(s.size) for s in streams]
    want = [PP.oracle_decode(p, n, 250) if n else (True, np.zeros(0, np.uint8)) for p, n in zip(pays, outs)]
    assert all(w[0] for w in want)
    _check(dec, pays, outs, want, name)


# ---- 2. hand-made payloads: one call per item, then all of them in one call ------------------------------------------------------------------------
@pytest.mark.parametrize("name", [it.name for it in CORPUS])
def test_hand_made_payload(dec, expected, name):
    it = next(i for i in CORPUS if i.name == name)
    ok, _ = expected[name]
    assert ok == it.valid
    _check(dec, [it.payload], [it.out_bytes], [expected[name]], name)


def test_whole_corpus_in_one_call(dec, expected):
    st, _ = _check(dec, [it.payload for it in CORPUS], [it.out_bytes for it in CORPUS], [expected[it.name] for it in CORPUS], "corpus")
    assert np.count_nonzero(st) == sum(not it.valid for it in CORPUS)


def test_truncation_boundary(dec, oracle_built):
    b = PP.truncation_boundary()
    counts = [2, 385, b, b + 1, b + 2]
    want = [PP.oracle_decode(PP.HEADER_ONLY, 3 * n, 250) for n in counts]
    assert [w[0] for w in want] == [True, True, True, False, False]
    _check(dec, [PP.HEADER_ONLY] * len(counts), [3 * n for n in counts], want, "header only")


# ---- 3. isolation: malformed streams are data ---------------------------------------------------------------------------------------------------------
def _raw_view(ptr, n):
    class _View:
        __cuda_array_interface__ = {"shape": (int(n),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    return _torch().as_tensor(_View(), device="cuda")


def test_64_streams_every_fourth_malformed_and_nothing_outside_the_slots(dec, expected):
    torch = _torch()
    good = [it for it in CORPUS if it.valid]
    bad = [it for it in CORPUS if not it.valid]
    items = [bad[(i // 4) % len(bad)] if i % 4 == 1 else good[(5 * i) % len(good)] for i in range(64)]
    pays, outs, want = [it.payload for it in items], [it.out_bytes for it in items], [expected[it.name] for it in items]
    _check(dec, pays, outs, want, "first run")                              # sizes the grow-only buffer
    views = [dec.palette_decoded_device(i) for i in range(64)]
    lo = min(v.data_ptr() for v in views)
    hi = max(v.data_ptr() + v.numel() for v in views)
    assert all(v.data_ptr() % 16 == 0 for v in views)
    spans = sorted((v.data_ptr(), v.data_ptr() + v.numel()) for v in views)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))              # packed, not overlapping
    dec.synchronize()
    whole = _raw_view(lo - 64, hi - lo + 128)
    whole.fill_(0xA5)
    torch.cuda.synchronize()
    st, got = _check(dec, pays, outs, want, "second run")                   # the same sizes: the buffer stays where it is
    assert np.count_nonzero(st) == 16
    assert [dec.palette_decoded_device(i).data_ptr() for i in range(64)] == [v.data_ptr() for v in views]
    after = whole.cpu().numpy()
    assert (after[:64] == 0xA5).all() and (after[-64:] == 0xA5).all()
    for (a, b), (c, _) in zip(spans, spans[1:]):                            # nor between the slots
        assert (after[b - lo + 64:c - lo + 64] == 0xA5).all()


# ---- 4. many, empty, changing counts, long ---------------------------------------------------------------------------------------------------------
def _many(n, seed):
    rng = np.random.default_rng(seed)
    pays, outs = [], []
    for i in range(n):
        k = int(rng.integers(0, 41))
        if k == 0 or i % 11 == 3:
            pays.append(np.zeros(0, np.uint8) if i % 2 else np.array([1, 2, 3, 4, 5, 6, 7], np.uint8)); outs.append(0)   # skipped, with or without bytes
        else:
            b = PP.random_stream(k, seed * 1000 + i)
            pays.append(b.payload()); outs.append(3 * k)
    return pays, outs


def test_448_streams_with_empties_then_3_then_449(dec, oracle_built):
    for n, seed in ((448, 1), (3, 2), (449, 3)):
        pays, outs = _many(n, seed)
        assert outs.count(0) > 0 or n == 3
        want = [PP.oracle_decode(p, o, 250) if o else (True, np.zeros(0, np.uint8)) for p, o in zip(pays, outs)]
        assert all(w[0] for w in want)
        _check(dec, pays, outs, want, n)


def test_300000_noise_colours_from_the_device_compressor(dec, enc, oracle_built):
    stream = PS.noise(300000, seed=31)
    t = _torch().from_numpy(stream.copy()).cuda()
    enc.palette_compress_streams([t], 1)
    pay = enc.palette_payload(0)
    ok, want = PP.oracle_decode(pay, stream.size, 250)
    assert ok
    dec.palette_decompress_streams([enc.palette_payload_device(0)], [stream.size], 250)      # where the encoder left it
    assert not dec.palette_status().any()
    _same(dec.palette_decoded(0), want, "300000 colours")
    _same(want, oracle_built.palette_remap(stream, 250), "noise round-trips")


# ---- 5. remap ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remap", [0, 1, 250, 255])
def test_remap_range(dec, oracle_built, remap):
    streams = [PS.ramp_noise(700, 5), PS.noise(1500, 6), PS.constant(3)]
    pays = PS.oracle_payloads(streams, 1)
    items = [it for it in CORPUS if it.valid][:12]
    pays += [it.payload for it in items]
    outs = [int(s.size) for s in streams] + [it.out_bytes for it in items]
    want = [PP.oracle_decode(p, o, remap) for p, o in zip(pays, outs)]
    _, got = _check(dec, pays, outs, want, ("remap", remap), remap)
    if remap == 0:                                                          # a clean round trip gives the encoder's stream back
        for s, g in zip(streams, got):
            _same(g, s, "remap 0 == the stream")
    else:                                                                   # remap 0 is not what the oracle does with range 0 (that is range 1's factor)
        raw = [PP.oracle_decode(p, o, 0)[1] for p, o in zip(pays, outs)]
        for r, w in zip(raw, want):
            _same(oracle_built.palette_remap(r, remap), w[1], "remap is applied behind the decode")


# ---- 6. handle behaviour ---------------------------------------------------------------------------------------------------------------------------
def test_stage_interval_views_and_host_copies(dec, expected):
    dec.stage_ms(YK_STAGE_PALETTE_DEC)                                      # drop what earlier tests recorded
    L, h = dec_lib(dec)
    items = [it for it in CORPUS if it.valid][:9]
    calls = 0
    for k in (9, 2, 5):
        sub = items[:k]
        dec.palette_decompress_streams(_dev([it.payload for it in sub]), [it.out_bytes for it in sub], 250)
        calls += 1
        assert not dec.palette_status().any()
        for i, it in enumerate(sub):
            w = expected[it.name][1]
            n = C.c_size_t()
            assert L.yk_palette_decoded(h, i, None, 0, C.byref(n)) == 0 and n.value == w.size
            buf = np.full(w.size + 32, 0xA5, np.uint8)
            assert L.yk_palette_decoded(h, i, buf.ctypes.data, buf.size, C.byref(n)) == 0 and n.value == w.size
            _same(buf[:w.size], w, ("host copy", i))
            assert (buf[w.size:] == 0xA5).all()
            assert L.yk_palette_decoded(h, i, buf.ctypes.data, w.size - 1, C.byref(n)) == YK_ERR_RANGE and n.value == w.size
            view = dec.palette_decoded_device(i)
            assert view.numel() == w.size and view.data_ptr() % 16 == 0
            _same(view.cpu().numpy(), w, ("device view", i))
    ms, n = dec.stage_ms(YK_STAGE_PALETTE_DEC)
    assert n == calls and ms > 0                                            # one interval per call


def dec_lib(d):
    from yaik_amd._lib import lib
    return lib(), d._h


def _refused(L, h, rc, code, text):
    msg = L.yk_last_error(h).decode()
    assert rc == code, (rc, code, msg)
    assert text in msg, msg


def test_refusals_leave_everything_as_it_was(expected):
    d = HipTileDecoder(0)
    try:
        L, h = dec_lib(d)
        dev_p, n_b = C.c_void_p(), C.c_size_t()
        st3 = (C.c_int32 * 3)()
        _refused(L, h, L.yk_palette_decoded_device(h, 0, C.byref(dev_p), C.byref(n_b)), YK_ERR_STATE, "first")
        _refused(L, h, L.yk_palette_decoded(h, 0, None, 0, C.byref(n_b)), YK_ERR_STATE, "first")
        _refused(L, h, L.yk_palette_decode_status(h, st3), YK_ERR_STATE, "first")
        items = [it for it in CORPUS if it.valid][3:6]
        dev = _dev([it.payload for it in items])
        d.palette_decompress_streams(dev, [it.out_bytes for it in items], 250)

        def unchanged(what):
            assert not d.palette_status().any()
            for i, it in enumerate(items):
                _same(d.palette_decoded(i), expected[it.name][1], (what, i))

        unchanged("valid call")
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in dev])
        lens = (C.c_size_t * 3)(*[t.numel() for t in dev])
        outs = (C.c_size_t * 3)(*[it.out_bytes for it in items])
        call = L.yk_palette_decompress_streams
        _refused(L, h, call(h, None, lens, outs, 3, 250), YK_ERR_BAD_ARG, "NULL")
        _refused(L, h, call(h, ptrs, None, outs, 3, 250), YK_ERR_BAD_ARG, "NULL")
        _refused(L, h, call(h, ptrs, lens, None, 3, 250), YK_ERR_BAD_ARG, "NULL")
        for n in (0, -1, 65537):
            _refused(L, h, call(h, ptrs, lens, outs, n, 250), YK_ERR_BAD_ARG, "nStreams")
        for r in (-1, 256):
            _refused(L, h, call(h, ptrs, lens, outs, 3, r), YK_ERR_BAD_ARG, "remapRange")
        for wrong in (outs[1] - 1, outs[1] + 1):
            _refused(L, h, call(h, ptrs, lens, (C.c_size_t * 3)(outs[0], wrong, outs[2]), 3, 250), YK_ERR_BAD_ARG, "multiple of 3")
        _refused(L, h, call(h, ptrs, (C.c_size_t * 3)(lens[0], 0, lens[2]), outs, 3, 250), YK_ERR_BAD_ARG, "empty payload")
        _refused(L, h, call(h, (C.c_void_p * 3)(ptrs[0], None, ptrs[2]), lens, outs, 3, 250), YK_ERR_BAD_ARG, "NULL pointer")
        _refused(L, h, call(h, ptrs, lens, (C.c_size_t * 3)(outs[0], 3 * ((1 << 28) + 1), outs[2]), 3, 250), YK_ERR_BAD_ARG, "2^28 colours")
        _refused(L, h, call(h, ptrs, lens, (C.c_size_t * 3)(3 << 27, 3 << 27, 3), 3, 250), YK_ERR_BAD_ARG, "2^28 colours")
        _refused(L, h, call(h, ptrs, (C.c_size_t * 3)(lens[0], (1 << 31) + 1, lens[2]), outs, 3, 250), YK_ERR_BAD_ARG, "2^31 payload bytes")
        _refused(L, h, call(h, ptrs, (C.c_size_t * 3)(1 << 30, 1 << 30, 1), outs, 3, 250), YK_ERR_BAD_ARG, "2^31 payload bytes")
        for i in (-1, 3):
            _refused(L, h, L.yk_palette_decoded_device(h, i, C.byref(dev_p), C.byref(n_b)), YK_ERR_BAD_ARG, "out of range")
            _refused(L, h, L.yk_palette_decoded(h, i, None, 0, C.byref(n_b)), YK_ERR_BAD_ARG, "out of range")
        _refused(L, h, L.yk_palette_decoded_device(h, 0, None, C.byref(n_b)), YK_ERR_BAD_ARG, "NULL")
        _refused(L, h, L.yk_palette_decode_status(h, None), YK_ERR_BAD_ARG, "NULL")
        # yk_decode_gradient_palette before yk_decode_begin
        bm = np.zeros(64, np.uint8)
        pay = items[0].payload
        _refused(L, h, L.yk_decode_gradient_palette(h, 4, 4, bm.ctypes.data, bm.size, pay.ctypes.data, pay.size, items[0].out_bytes, 250), YK_ERR_STATE, "yk_decode_begin")
        unchanged("after the refusals")
        # a skipped stream may have no pointer and no bytes
        assert call(h, (C.c_void_p * 3)(ptrs[0], None, ptrs[2]), (C.c_size_t * 3)(lens[0], 0, lens[2]), (C.c_size_t * 3)(outs[0], 0, outs[2]), 3, 250) == 0
        assert not d.palette_status().any() and d.palette_decoded(1).size == 0
        _same(d.palette_decoded(2), expected[items[2].name][1], "behind a skipped stream")
    finally:
        d.close()


# ---- 7. the 'GTIL' payload in front of the gradient decode ---------------------------------------------------------------------------------------------
def _encode(e, planes):
    e.set_image(planes)
    if planes.shape[0] == 4:
        e.mip_prefilter()
    e.encode(3, False)


def test_decode_gradient_palette_equals_decode_gradient_and_refuses_a_malformed_payload(enc, oracle_built):
    planes = edge_image(136, 72, "mixed", 3, seed=8)
    _encode(enc, planes)
    raw = [enc.gradient_corners(p) for p in range(7)]
    bms = [enc.gradient_bitmap(p) for p in range(7)]
    pays = PS.oracle_payloads(raw, 7)
    a, b = HipTileDecoder(0), HipTileDecoder(0)
    try:
        L = dec_lib(a)[0]
        a.begin(136, 72); b.begin(136, 72)
        used = 0
        for p, (sx, sy) in enumerate([(4, 4), (4, 3), (3, 4), (3, 3), (3, 2), (2, 3), (2, 2)]):
            if not raw[p].size:
                continue
            ok, rgb = PP.oracle_decode(pays[p], raw[p].size, 250)
            assert ok
            a.decompress_gradient(sx, sy, bms[p], rgb)
            rc = L.yk_decode_gradient_palette(b._h, sx, sy, bms[p].ctypes.data, bms[p].size, pays[p].ctypes.data, pays[p].size, raw[p].size, 250)
            assert rc == 0, L.yk_last_error(b._h)
            used += 1
            assert np.array_equal(a.planes(), b.planes()) and np.array_equal(a.tile4x4(), b.tile4x4()), p
        assert used >= 2
        # a malformed payload: refused with a message, and the image is as it was
        before, before4 = b.planes().copy(), b.tile4x4().copy()
        p = next(q for q in range(7) if raw[q].size)
        bad = pays[p].copy()
        bad[4 + 3 * int(bad[0])] = 0x97                                     # the first token becomes an extension code
        assert not PP.oracle_decode(bad, raw[p].size)[0]
        rc = L.yk_decode_gradient_palette(b._h, 4, 4, bms[0].ctypes.data, bms[0].size, bad.ctypes.data, bad.size, raw[p].size, 250)
        _refused(L, b._h, rc, YK_ERR_BAD_ARG, "malformed")
        assert np.array_equal(b.planes(), before) and np.array_equal(b.tile4x4(), before4)
    finally:
        a.close(); b.close()


def _planes_equal(a, b, frames=1):
    for f in range(frames):
        if frames > 1:
            a.select_frame(f); b.select_frame(f)
        assert np.array_equal(a.planes(), b.planes()), f
        assert np.array_equal(a.tile4x4(), b.tile4x4()), f


@pytest.mark.parametrize("name", ["synth256_rgba", "mixed128_rgba"])
def test_decode_from_encoder_through_the_payloads(enc, name):
    from tests.golden.make_golden import FULL
    planes = FULL[name]()
    _encode(enc, planes)
    h, w = planes.shape[1:]
    a, b = HipTileDecoder(0), HipTileDecoder(0)
    try:
        a.begin(w, h); b.begin(w, h)
        a.decode_from_encoder(enc)
        with pytest.raises(ValueError, match="palette_compress"):          # the payloads are the caller's to make
            b.decode_from_encoder(enc, palette=True)
        enc.palette_reset()                                                 # like the first image of a file
        enc.palette_compress()
        b.decode_from_encoder(enc, palette=True)
        _planes_equal(a, b)
        assert b.palette_status().size > 0 and not b.palette_status().any()
    finally:
        a.close(); b.close()


def _u8(images):
    return _torch().from_numpy(np.ascontiguousarray(np.stack([np.moveaxis(p, 0, -1) for p in images]).astype(np.uint8))).cuda()


@pytest.mark.parametrize("side,n", [(64, 3), (16, 33)])
def test_decode_batch_from_encoder_through_the_payloads(enc, side, n):
    kinds = ("mixed", "synth", "smooth", "twocolor", "ramp")
    images = [edge_image(side, side, kinds[f % len(kinds)], 3, seed=3 + f) if kinds[f % len(kinds)] != "synth" else synth_planes(side, n_planes=3)
              for f in range(n)]
    enc.set_batch_u8(_u8(images))
    enc.encode_batch(3, False)
    a, b = HipTileDecoder(0), HipTileDecoder(0)
    try:
        a.begin_batch(side, side, n); b.begin_batch(side, side, n)
        a.decode_batch_from_encoder(enc)
        with pytest.raises(ValueError, match="palette_compress_batch"):    # a.decode... built a new table: no payloads of it yet
            b.decode_batch_from_encoder(enc, palette=True)
        enc.palette_compress_batch()
        b.decode_batch_from_encoder(enc, palette=True)
        assert b.palette_status().size > 0 and not b.palette_status().any()
        assert _torch().equal(a.image_batch_device(), b.image_batch_device())
        _planes_equal(a, b, n)
    finally:
        a.close(); b.close()


def test_a_rejected_payload_raises_on_the_encoder_path(dec):
    """_through_palette raises when PaletteDecompressor rejects a payload: here the encoder's payload view is replaced by a malformed one."""
    bad = next(it for it in CORPUS if not it.valid)

    class _Enc:
        def palette_payload_device(self, i):
            return _dev([bad.payload])[0]

    with pytest.raises(YaikError, match="rejects"):
        dec._through_palette(_Enc(), [[("g", 4, 4, 1, 1, 1, bad.out_bytes)]])
