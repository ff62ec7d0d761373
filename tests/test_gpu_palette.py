"""PaletteCompressor on the GPU (yk_palette_*; HipTileEncoder.palette_*): every payload byte for byte against the CPU oracle called in the same
order (so that the carried code-book rows are the same), against the compiled reference's fixtures, against the single-image path, and, above
the oracle's stream limit, against the host coder (yaik_amd/host/palette.cpp through entropy_tool).  The hand-made streams, and the proof that
they reach every token kind, are in tests/palette_streams.py and tests/test_palette_layout.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import palette_streams as PS
from tests.images import edge_image, synth_planes
from yaik_amd.encoder import HipTileEncoder

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_ERR_RANGE = -2, -4, -5
YK_STAGE_PALETTE = 9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = PS.cases()


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def enc():
    e = HipTileEncoder(0)
    yield e
    e.close()


def _dev(streams):
    t = _torch()
    return [t.from_numpy(s.copy()).cuda() if s.size else t.empty(0, dtype=t.uint8, device="cuda") for s in streams]


def _same(got, want, what):
    assert got.size == want.size, (what, "length", got.size, want.size)
    if not np.array_equal(got, want):
        first = int(np.argmax(got != want))
        raise AssertionError((what, "first difference at byte", first, got[max(0, first - 4):first + 8].tolist(), want[max(0, first - 4):first + 8].tolist()))


def _run(e, streams, chain):
    n = e.palette_compress_streams(_dev(streams), chain)
    assert n == len(streams)
    return [e.palette_payload(i) for i in range(n)]


# ---- 1. hand-made streams: lengths around the workgroup size, every content, every chain -----------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_hand_made_streams_match_the_oracle(enc, oracle_built, name):
    _, streams, chain = next(c for c in CASES if c[0] == name)
    want = PS.oracle_payloads(streams, chain)
    got = _run(enc, streams, chain)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (name, i, streams[i].size // 3))


def test_chain_zero_continues_across_calls_and_reset_forgets(enc, oracle_built):
    a, b, c = PS.stale_pair()
    ora = PS._oracle()
    enc.palette_reset()
    first = _run(enc, [a, b], 0)                                            # b sees a's stale rows
    second = _run(enc, [c, b], 0)                                           # the next call continues where the first stopped
    want = PS.oracle_payloads([a, b, c, b], 0, ora)
    for i, g in enumerate(first + second):
        _same(g, want[i], ("continued", i))
    enc.palette_reset()
    fresh = _run(enc, [b, c], 0)
    want_fresh = PS.oracle_payloads([b, c], 0, PS._oracle())
    for i, g in enumerate(fresh):
        _same(g, want_fresh[i], ("after reset", i))
    assert not np.array_equal(fresh[0], first[1])                           # the stale rows did matter
    # a chained call in between neither reads nor writes the carried rows
    enc.palette_reset()
    _run(enc, [a], 0)
    _run(enc, [c, c], 2)
    _same(_run(enc, [b], 0)[0], first[1], "carried rows survive a chained call")
    enc.palette_reset()


# ---- 2. real frames ------------------------------------------------------------------------------------------------------------------------
def _encode(e, planes):
    e.set_image(planes)
    if planes.shape[0] == 4:
        e.mip_prefilter()
    e.encode(3, False)


@pytest.mark.parametrize("name", ["synth256_rgba", "mixed128_rgba", "synth64_rgb", "ramp72x40_rgb"])
def test_frames_match_the_oracle_and_the_compiled_reference(enc, oracle_built, name):
    """The fixtures tests/golden/<name>.npz hold grad_palette_<pass> as the compiled reference wrote it (tests/blobs.py, tests/golden/make_golden.py)."""
    from tests.golden.make_golden import FULL
    planes = FULL[name]()
    _encode(enc, planes)
    raw = [enc.gradient_corners(p) for p in range(7)]
    ora = PS._oracle()
    want = PS.oracle_payloads(raw, 0, ora)
    enc.palette_reset()
    assert enc.palette_compress() == 7
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    seen = 0
    for p in range(7):
        got = enc.palette_payload(p)
        _same(got, want[p], (name, "oracle", p))
        key = f"grad_palette_{p}"
        if raw[p].size:
            assert key in z.files, (name, p)
            _same(got, z[key], (name, "compiled reference", p))
            seen += 1
    assert seen > 0
    # the second frame of a process continues the book: the same frame again, without a reset
    assert enc.palette_compress() == 7
    again = PS.oracle_payloads(raw, 0, ora)
    for p in range(7):
        _same(enc.palette_payload(p), again[p], (name, "continued", p))
    enc.palette_reset()


def _u8(images):
    return _torch().from_numpy(np.ascontiguousarray(np.stack([np.moveaxis(p, 0, -1) for p in images]).astype(np.uint8))).cuda()


@pytest.mark.parametrize("side,n", [(64, 3), (16, 33)])
def test_batch_equals_single_images_from_a_reset_book(enc, oracle_built, side, n):
    kinds = ("mixed", "synth", "smooth", "twocolor", "ramp")
    images = [edge_image(side, side, kinds[f % len(kinds)], 3, seed=3 + f) if kinds[f % len(kinds)] != "synth" else synth_planes(side, n_planes=3)
              for f in range(n)]
    enc.set_batch_u8(_u8(images))
    enc.encode_batch(3, False)
    rows = enc.streams_batch(corners=True, range1d=False)
    assert enc.palette_compress_batch() == 7 * n
    batch = [enc.palette_payload(i) for i in range(7 * n)]
    assert sum(b.size for b in batch) > 0
    for f in range(n):
        raw = rows[f].download()["rgb"]
        want = PS.oracle_payloads(raw, 7)
        for p in range(7):
            _same(batch[f * 7 + p], want[p], (side, "oracle", f, p))
    for f in range(n):                                                      # the single-image call, every frame from a reset book
        enc.select_frame(f)
        enc.palette_reset()
        assert enc.palette_compress() == 7
        for p in range(7):
            _same(enc.palette_payload(p), batch[f * 7 + p], (side, "single", f, p))
    enc.palette_reset()


# ---- 3. above the oracle's limit of 99 998 colours: the host coder ------------------------------------------------------------------------------
def test_long_stream_matches_the_host_coder(enc):
    from tests import chunks
    tool = chunks.build_tool()
    stream = PS.ramp_noise(300000, seed=9)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in"), "wb") as f:
            f.write(stream.tobytes())
        subprocess.run([tool, "palette", os.path.join(d, "out"), os.path.join(d, "in")], check=True, stdout=subprocess.DEVNULL)
        want = np.fromfile(os.path.join(d, "out0"), dtype=np.uint8)
    got = _run(enc, [stream], 1)[0]
    _same(got, want, "300000 colours")
    assert want.size < stream.size                                          # it compresses


# ---- 4. handle behaviour -------------------------------------------------------------------------------------------------------------------
def test_payload_extent_stage_intervals_and_changing_segment_counts(enc, oracle_built):
    enc.stage_ms(YK_STAGE_PALETTE)                                          # drop what earlier tests recorded
    L, h = enc._L, enc._h
    calls = 0
    for streams, chain in (([PS.noise(70, 1)], 1), (CASES[0][1][:14], 7), ([PS.ramp(5), PS.noise(300, 2), PS.constant(9)], 0), ([PS.ramp_noise(40)], 1)):
        want = PS.oracle_payloads(streams, chain)
        enc.palette_reset()
        dev = _dev(streams)
        assert enc.palette_compress_streams(dev, chain) == len(streams)
        calls += 1
        spans = []
        for i, w in enumerate(want):
            n = C.c_size_t()
            assert L.yk_palette_payload(h, i, None, 0, C.byref(n)) == 0 and n.value == w.size
            buf = np.full(w.size + 32, 0xA5, np.uint8)                      # sentinels behind the payload
            assert L.yk_palette_payload(h, i, buf.ctypes.data, buf.size, C.byref(n)) == 0 and n.value == w.size
            _same(buf[:w.size], w, ("host copy", i))
            assert (buf[w.size:] == 0xA5).all()
            if w.size:
                assert L.yk_palette_payload(h, i, buf.ctypes.data, w.size - 1, C.byref(n)) == YK_ERR_RANGE and n.value == w.size
                assert (buf[w.size:] == 0xA5).all()
            view = enc.palette_payload_device(i)
            assert view.numel() == w.size
            if w.size:
                assert view.data_ptr() % 16 == 0
                spans.append((view.data_ptr(), view.data_ptr() + w.size))
                enc.synchronize()
                _same(view.cpu().numpy(), w, ("device view", i))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))          # packed, not overlapping
        for s, t in zip(streams, dev):                                      # the inputs are only read
            assert np.array_equal(t.cpu().numpy(), s)
    ms, n = enc.stage_ms(YK_STAGE_PALETTE)
    assert n == calls and ms > 0                                            # one interval per call
    enc.palette_reset()


def _refused(e, rc, code, text):
    assert rc == code, (rc, code, e._L.yk_last_error(e._h))
    msg = e._L.yk_last_error(e._h).decode()
    assert text in msg, msg


def test_refusals_leave_everything_as_it_was(oracle_built):
    e = HipTileEncoder(0)
    try:
        L, h = e._L, e._h
        dev_p, n_b = C.c_void_p(), C.c_size_t()
        # the getters before any call; compress before an encode; batch without a table
        _refused(e, L.yk_palette_payload_device(h, 0, C.byref(dev_p), C.byref(n_b)), YK_ERR_STATE, "first")
        _refused(e, L.yk_palette_payload(h, 0, None, 0, C.byref(n_b)), YK_ERR_STATE, "first")
        _refused(e, L.yk_palette_compress(h), YK_ERR_STATE, "yk_encode_tiles first")
        _refused(e, L.yk_palette_compress_batch(h), YK_ERR_STATE, "YK_STREAMS_CORNERS")
        # a valid call, whose payloads must survive every refusal below
        a, b, c = PS.stale_pair()
        streams = [a, b, c]
        want = PS.oracle_payloads(streams, 0, PS._oracle())
        dev = _dev(streams)
        e.palette_compress_streams(dev, 0)

        def unchanged(what):
            for i, w in enumerate(want):
                _same(e.palette_payload(i), w, (what, i))

        unchanged("valid call")
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in dev])
        lens = (C.c_size_t * 3)(*[t.numel() for t in dev])
        _refused(e, L.yk_palette_compress_streams(h, None, lens, 3, 0), YK_ERR_BAD_ARG, "NULL")
        _refused(e, L.yk_palette_compress_streams(h, ptrs, None, 3, 0), YK_ERR_BAD_ARG, "NULL")
        for n in (0, -1, 65537):
            _refused(e, L.yk_palette_compress_streams(h, ptrs, lens, n, 0), YK_ERR_BAD_ARG, "nStreams")
        _refused(e, L.yk_palette_compress_streams(h, ptrs, lens, 3, -1), YK_ERR_BAD_ARG, "chain")
        bad = (C.c_size_t * 3)(lens[0], lens[1] - 1, lens[2])
        _refused(e, L.yk_palette_compress_streams(h, ptrs, bad, 3, 0), YK_ERR_BAD_ARG, "multiple of 3")
        nul = (C.c_void_p * 3)(ptrs[0], None, ptrs[2])
        _refused(e, L.yk_palette_compress_streams(h, nul, lens, 3, 0), YK_ERR_BAD_ARG, "NULL pointer")
        for i in (-1, 3):
            _refused(e, L.yk_palette_payload_device(h, i, C.byref(dev_p), C.byref(n_b)), YK_ERR_BAD_ARG, "out of range")
            _refused(e, L.yk_palette_payload(h, i, None, 0, C.byref(n_b)), YK_ERR_BAD_ARG, "out of range")
        _refused(e, L.yk_palette_payload_device(h, 0, None, C.byref(n_b)), YK_ERR_BAD_ARG, "NULL")
        _refused(e, L.yk_palette_compress(h), YK_ERR_STATE, "yk_encode_tiles first")
        _refused(e, L.yk_palette_compress_batch(h), YK_ERR_STATE, "YK_STREAMS_CORNERS")
        unchanged("after the refusals")
        # the carried rows were not touched either: b again continues a, b, c exactly like the oracle
        ora = PS._oracle()
        PS.oracle_payloads(streams, 0, ora)
        _same(_run(e, [b], 0)[0], PS.oracle_payloads([b], 0, ora)[0], "carried rows after the refusals")
        # a stripe
        big = edge_image(64, 128, "mixed", 3, seed=3)
        e.set_image(big[:, :65], full_h=128, y0=0, halo_rows=1)
        e.encode(3, False)
        _refused(e, L.yk_palette_compress(h), YK_ERR_STATE, "stripe")
        # a streams table without corner streams, then a refused call on a valid table: the table and its streams stay
        images = [edge_image(72, 40, k, 3, seed=5) for k in ("mixed", "smooth")]
        e.set_batch_u8(_u8(images))
        e.encode_batch(3, False)
        e.streams_batch(corners=False, range1d=True)
        _refused(e, L.yk_palette_compress_batch(h), YK_ERR_STATE, "YK_STREAMS_CORNERS")
        rows = e.streams_batch(corners=True, range1d=True)
        before = [r.download() for r in rows]
        assert e.palette_compress_batch() == 14
        pay = [e.palette_payload(i) for i in range(14)]
        _refused(e, L.yk_palette_compress_streams(h, ptrs, lens, 3, -7), YK_ERR_BAD_ARG, "chain")
        _refused(e, L.yk_palette_payload(h, 14, None, 0, C.byref(n_b)), YK_ERR_BAD_ARG, "out of range")
        from yaik_amd.encoder import _FrameStreamsC
        tab = (_FrameStreamsC * 2)()
        assert L.yk_batch_streams_table(h, tab) == 0 and [int(t.pix or 0) for t in tab] == [r.pix for r in rows]
        for r, was in zip(rows, before):
            now = r.download()
            assert all(np.array_equal(x, y) for x, y in zip(now["rgb"], was["rgb"])) and np.array_equal(now["pix"], was["pix"])
        for i, p in enumerate(pay):
            _same(e.palette_payload(i), p, ("batch payloads after a refusal", i))
        for f in range(2):
            want_f = PS.oracle_payloads(before[f]["rgb"], 7)
            for p in range(7):
                _same(pay[f * 7 + p], want_f[p], ("batch", f, p))
        # a new encode invalidates the payloads, like the table
        e.encode_batch(3, False)
        _refused(e, L.yk_palette_payload(h, 0, None, 0, C.byref(n_b)), YK_ERR_STATE, "first")
        # after a plane-subset pass
        pm = edge_image(64, 64, "planemix", 3, seed=2)
        e.set_image(pm)
        e.encode(3, False)
        e.fitting_quad_smooth_planes(3, 2, 2)
        _refused(e, L.yk_palette_compress(h), YK_ERR_STATE, "plane-subset")
        # and the handle still works
        e.set_image(edge_image(64, 64, "mixed", 3, seed=4))
        e.encode(3, False)
        raw = [e.gradient_corners(p) for p in range(7)]
        e.palette_reset()
        e.palette_compress()
        want = PS.oracle_payloads(raw, 7)
        for p in range(7):
            _same(e.palette_payload(p), want[p], ("afterwards", p))
    finally:
        e.close()
