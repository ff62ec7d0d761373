"""Directed tests of the live 1-D range coder (yk_range1d.hip: DynamicTileCompressor, the '1DTL' chunk) and of its decoder (yk_dec1d_* in
yk_decode.hip) on images whose gradient coverage is set cell by cell (tests/range1d_cases.py; tests/test_range1d_cases.py shows from the reference
alone that every case holds what it claims).  Every comparison is byte for byte against the CPU oracle.

Encoder: the coder's sparse path (a 64x16 strip with at most four uncovered cells) and its dense path, every quadrant pattern 1..15 in both, the
partial last strip column and row, tiles behind the first scan block of 1024 and a scan block that is completely uncovered; in the four builds of
the body: from the planes, from the fused kernel's pixel cache, per-plane slots + pack after plane-subset passes, and the batch kernel.  G and B
carry the value regimes (mode clamps, delta 0 / 1 / 2 / 3 / 255, ties, a tile with all 17 bytes).
Decoder: the same streams through yk_decode_1d (shared and per-plane masks), yk_decode_1d_device and the batch entry: every branch of a half
tile (both quadrants, one, none) with known patterns."""
import functools

import numpy as np
import pytest

from oracle.pyoracle import PASSES, OracleDecoder, palette_remap
from tests import range1d_cases as rc
from tests.blobs import PP_MASKS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hip_batch():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=[2, 1], ids=["kernel_v2", "kernel_v1"])
def hip_gen(request):
    """both generations of the fused kernel: the coverage the coder reads comes from it"""
    from tests.parity import encoder_for_kernel_version
    e = encoder_for_kernel_version(request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dec():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


def _same_streams(pix, typ, run, what):
    """type stream first: a wrong triple names the tile, a wrong pixel byte its offset"""
    assert (typ.size, pix.size) == (run["type"].size, run["pix"].size), (what, "stream lengths", typ.size, pix.size, run["type"].size, run["pix"].size)
    if not np.array_equal(typ, run["type"]):
        i = int(np.nonzero(typ != run["type"])[0][0])
        raise AssertionError((what, "parameter triple of coded tile", i // 3, typ[i // 3 * 3: i // 3 * 3 + 3].tolist(), run["type"][i // 3 * 3: i // 3 * 3 + 3].tolist()))
    if not np.array_equal(pix, run["pix"]):
        bad = np.nonzero(pix != run["pix"])[0]
        raise AssertionError((what, "pixel stream", int(bad.size), "bytes differ, first at", int(bad[0])))


def _encode(e, c, what):
    e.set_image(c["planes"])
    e.encode(3, False, False)
    assert np.array_equal(e.coverage(), ~c["run"]["shared"]), (what, "coverage of the fused kernel")


# ---- encoder builds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.SHARED_NAMES)
def test_from_the_planes(hip_gen, oracle_built, name):
    c = rc.case(name)
    _encode(hip_gen, c, name)
    pix, typ = hip_gen.dynamic_tile_compressor()
    _same_streams(pix, typ, c["run"], name)


@pytest.mark.parametrize("name", rc.SHARED_NAMES)
def test_from_the_pixel_cache(hip, oracle_built, name):
    c = rc.case(name)
    hip.set_pixel_cache(True)
    try:
        _encode(hip, c, name)
        pix, typ = hip.dynamic_tile_compressor()
        _same_streams(pix, typ, c["run"], (name, "pixel cache"))
    finally:
        hip.set_pixel_cache(False)


def _per_plane_encode(e, c, what):
    _encode(e, c, what)
    for m, (cnt, bm, rgb) in zip(PP_MASKS, c["run"]["pp"]):
        gcnt, gbm, grgb = e.fitting_quad_smooth_planes(m)
        assert gcnt == cnt and np.array_equal(gbm, bm) and np.array_equal(grgb, rgb), (what, "plane-subset pass", m, gcnt, cnt)
    for p in range(3):
        assert np.array_equal(e.coverage_plane(p), ~c["run"]["uncovered"][p]), (what, "coverage of plane", p)


@pytest.mark.parametrize("name", rc.PER_PLANE_NAMES)
def test_per_plane_slots_and_pack(hip, oracle_built, name):
    c = rc.case(name)
    _per_plane_encode(hip, c, name)
    pix, typ = hip.dynamic_tile_compressor()
    _same_streams(pix, typ, c["run"], name)


@functools.lru_cache(maxsize=None)
def _values_after_subset_passes():
    c = dict(rc.case("s264x136_flat"))
    c["run"] = rc.oracle_run(c["planes"], per_plane=True)
    return c


def test_per_plane_form_with_the_value_regimes(hip, oracle_built):
    """the shared-coverage image with the value cells, after the plane-subset passes: R keeps its plugs, G and B keep the cells whose values no 4x4
    tile fits, so the slot + pack form meets the regimes too"""
    c = _values_after_subset_passes()
    unc = c["run"]["uncovered"]
    assert unc[1].any() and not np.array_equal(unc[0], unc[1]) and not np.array_equal(unc[1], unc[2])
    assert {(1, rc.FLAT, 0), (254, rc.FLAT, 0), (rc.FLAT, 0, 255)} <= rc.census(c["planes"], True, c["run"])["triples"]
    _per_plane_encode(hip, c, "values")
    pix, typ = hip.dynamic_tile_compressor()
    _same_streams(pix, typ, c["run"], "values")


@pytest.mark.parametrize("bname", sorted(rc.BATCHES))
def test_batch(hip_batch, dec, oracle_built, bname):
    """three different layouts of one shape as one batch: every frame's streams, in frame order, with its own totals; then the batch decoder on them"""
    import torch
    cases = [rc.case(n) for n in rc.BATCHES[bname]]
    frames = torch.from_numpy(np.ascontiguousarray(np.stack([c["planes"] for c in cases]))).cuda()
    h, w = cases[0]["planes"].shape[1:]
    hip = hip_batch
    hip.set_batch(frames)
    hip.encode_batch(3, False)
    rows = hip.streams_batch(corners=False, range1d=True)
    assert len(rows) == 3
    for f, (row, c) in enumerate(zip(rows, cases)):
        assert (row.pix_bytes, row.type_bytes) == (c["run"]["pix"].size, c["run"]["type"].size), (bname, f)
        got = row.download()
        _same_streams(got["pix"], got["type"], c["run"], (bname, "frame", f))
    dec.begin_batch(w, h, 3)
    dec.decode_batch_from_encoder(hip)
    for f, c in enumerate(cases):
        dec.select_frame(f)
        planes, t4 = _oracle_decode(c["name"])
        assert np.array_equal(dec.planes(), planes), (bname, "decoded frame", f)
        assert np.array_equal(dec.tile4x4(), t4), (bname, "tile4x4Mask of frame", f)


# ---- decoder -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_decode(name):
    """(planes, tile4x4Mask of plane 0) of the reference decoder on the reference encoder's streams of a shared-coverage case"""
    c = rc.case(name)
    h, w = c["planes"].shape[1:]
    od = OracleDecoder(w, h)
    for (sx, sy), (cnt, bm, rgb) in zip(PASSES, c["run"]["grad"]):
        if cnt:
            od.gradient(sx, sy, bm, palette_remap(rgb, 250))
    t4 = od.tile4x4()
    od.split_masks()
    assert od.decode_1d(c["run"]["type"], c["run"]["pix"]) == (c["run"]["type"].size, c["run"]["pix"].size)
    return od.planes(), t4


@pytest.mark.parametrize("name", rc.SHARED_NAMES)
def test_decode_shared_coverage(hip, dec, oracle_built, name):
    c = rc.case(name)
    h, w = c["planes"].shape[1:]
    _encode(hip, c, name)
    od = OracleDecoder(w, h)
    dec.begin(w, h)
    counts = hip.gradient_counts()
    for i, (sx, sy) in enumerate(PASSES):
        if counts[i]:
            bm, dq = hip.gradient_bitmap(i), palette_remap(hip.gradient_corners(i), 250)
            od.gradient(sx, sy, bm, dq)
            dec.decompress_gradient(sx, sy, bm, dq)
    pix, typ = hip.dynamic_tile_compressor()
    dec.decompress_1d(typ, pix)
    assert np.array_equal(dec.tile4x4(), od.tile4x4())
    od.split_masks()
    assert od.decode_1d(typ, pix) == (typ.size, pix.size)
    assert np.array_equal(dec.planes(), od.planes()), name
    assert np.array_equal(od.planes(), _oracle_decode(name)[0])
    # the coded pixels come back as the reference's DecompModel1 leaves them: a pixel of a value cell that coded as byte 0 is color0
    got = np.stack([dec.planes()[p].reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w) for p in range(3)])
    rec = {(p, ty, tx): triple for p, ty, tx, pat, kind, triple, b in rc.census(c["planes"], False, c["run"])["records"]}
    for p, ty, tx, regime, triple in c["expect"]:
        if regime == "within1":
            tile, unc = got[p, 8 * ty: 8 * ty + 8, 8 * tx: 8 * tx + 8], np.kron(c["want"][p, 2 * ty: 2 * ty + 2, 2 * tx: 2 * tx + 2], np.ones((4, 4), bool))
            assert rec[(p, ty, tx)] == triple and (tile[unc.astype(bool)] == triple[0]).all(), (name, regime, ty, tx)


@pytest.mark.parametrize("name", rc.PER_PLANE_NAMES)
def test_decode_per_plane_coverage(hip, dec, oracle_built, name):
    """the sequence of test_partial_round_trip_consistent_marks: per-plane masks, one decode launch per plane (planeOverride)"""
    c = rc.case(name)
    h, w = c["planes"].shape[1:]
    _encode(hip, c, name)
    od = OracleDecoder(w, h)
    dec.begin(w, h)
    counts = hip.gradient_counts()
    for i, (sx, sy) in enumerate(PASSES):
        if counts[i]:
            bm, dq = hip.gradient_bitmap(i), palette_remap(hip.gradient_corners(i), 250)
            od.gradient(sx, sy, bm, dq)
            dec.decompress_gradient(sx, sy, bm, dq)
    od.split_masks()
    for m in PP_MASKS:
        cnt, bm, rgb = hip.fitting_quad_smooth_planes(m)
        if cnt:
            dq = palette_remap(rgb, 250)
            od.gradient_planes(m, bm, dq, consistent_marks=True)
            dec.decompress_gradient_planes(m, bm, dq, consistent_marks=True)
    assert np.array_equal(dec.tile4x4(True).ravel(), od.tile4x4(True).ravel())
    pix, typ = hip.dynamic_tile_compressor()
    _same_streams(pix, typ, c["run"], name)
    assert od.decode_1d(typ, pix) == (typ.size, pix.size)
    dec.decompress_1d(typ, pix)
    assert np.array_equal(dec.planes(), od.planes()), name
    assert np.array_equal(dec.tile4x4(True).ravel(), od.tile4x4(True).ravel())


def test_decode_from_device_streams(hip, dec, oracle_built):
    """yk_decode_1d_device on a layout of sparse strips that reaches into the second scan block, the streams read where the coder left them"""
    name = "s264x264_sparse"
    c = rc.case(name)
    h, w = c["planes"].shape[1:]
    _encode(hip, c, name)
    planes, t4 = _oracle_decode(name)
    for per_pass in (False, True):
        dec.begin(w, h)
        dec.decode_from_encoder(hip, per_pass=per_pass)
        assert np.array_equal(dec.planes(), planes), per_pass
        assert np.array_equal(dec.tile4x4(), t4), per_pass


# ---- handle reuse ----------------------------------------------------------------------------------------------------------------------------------
def test_handle_reuse_dense_sparse_dense(oracle_built):
    """a dense case, a sparse case of a smaller shape, the dense case again on ONE handle: no offset, block sum or slot of the earlier image survives"""
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    try:
        first = None
        for step, name in enumerate(("s264x264_flat", "s72x40_ramp", "s264x264_flat")):
            c = rc.case(name)
            _encode(e, c, (step, name))
            pix, typ = e.dynamic_tile_compressor()
            _same_streams(pix, typ, c["run"], (step, name))
            if step == 0:
                first = (pix.copy(), typ.copy())
        assert np.array_equal(pix, first[0]) and np.array_equal(typ, first[1])
        # and through the per-plane form and back: the slots and counts of the plane-subset run do not leak into the direct form
        c = rc.case("pp72x40")
        _per_plane_encode(e, c, "pp72x40")
        pix, typ = e.dynamic_tile_compressor()
        _same_streams(pix, typ, c["run"], "pp72x40 on the reused handle")
        c = rc.case("s72x40_flat")
        _encode(e, c, "s72x40_flat")
        pix, typ = e.dynamic_tile_compressor()
        _same_streams(pix, typ, c["run"], "s72x40_flat after the per-plane form")
    finally:
        e.close()
