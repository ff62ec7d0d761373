"""Directed tests of the gradient passes of the fused encode kernel (y2_grad_pass in yk_encode2.hip) and of the first-generation cross-check
kernel (tests/csrc/yk_encode_v1.hip) on images built tile by tile (tests/gradfit_cases.py; tests/test_gradfit_cases.py shows from the reference
alone that every case holds what it claims).  Every comparison is bit for bit against the CPU oracle.

What the cases pin: every (shape, variant) as the sole survivor of a tile in the compact, the screened and (16x16) the smooth path; the deciding
pixel of the last variant at rf / rf + 1 in every row of a cell, both end columns, first and last cell, every stream; strips on both sides of the
compact threshold; the curvature bound at 4 rf + 1 / 4 rf + 2; corner values at the ends of the byte range and a saturated D; reject factors 0, 1
and 64; tiles whose corners are clamped reads at the right and bottom edge.  A mismatch names the case, the pass and, through the census, the
tile, its path and its survivor set."""
import numpy as np
import pytest

from tests import gradfit_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[2, 1], ids=["kernel_v2", "kernel_v1"])
def hip_gen(request):
    from tests.parity import encoder_for_kernel_version
    e = encoder_for_kernel_version(request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hip():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


def _tile_story(c, p, ty, tx):
    """what the census knows of a tile: target record (if it is one), path, survivors, where its last variant died"""
    rec = c["census"]["tiles"].get((p, ty, tx))
    tgt = [{k: v for k, v in t.items() if k in ("group", "expect", "variant", "decide", "kind", "curve", "edge", "count", "tl", "sat")}
           for t in c["targets"] if gc.target_tile(t) == (p, ty, tx)]
    if rec is None:
        return ("not viable under the kernel's rule", tgt)
    return ("path", rec["path"], "survivors", rec["survivors"], "oracle accepts" if rec["accepted"] else "oracle rejects", "last variant died at", rec["last"], tgt)


def _same_gradient(e, c, what):
    """type first (which pass, which tile, what the census says of it), detail second"""
    cs = c["census"]
    h, w = c["planes"].shape[1:]
    for p in range(7):
        cnt, bm, _ = cs["grad"][p]
        got = e.gradient_bitmap(p)
        assert got.size == bm.size, (what, "bitmap size of pass", p, got.size, bm.size)
        if not np.array_equal(got, bm):
            a, b = gc.bitmap_tiles(got, p, w, h), gc.bitmap_tiles(bm, p, w, h)
            bad = np.argwhere(a != b)
            if len(bad):
                ty, tx = (int(v) for v in bad[0])
                raise AssertionError((what, "pass", p, gc.SHAPES[p], "tile", (ty, tx), "kernel accepts" if a[ty, tx] else "kernel rejects", len(bad), "tiles differ") + _tile_story(c, p, ty, tx))
            raise AssertionError((what, "pass", p, "bitmap bits outside the image differ"))
    assert e.gradient_counts().tolist() == [g[0] for g in cs["grad"]], (what, "counts")
    assert np.array_equal(e.coverage(), cs["coverage"]), (what, "coverage")
    for p in range(7):
        got, want = e.gradient_corners(p), cs["grad"][p][2]
        assert got.size == want.size and np.array_equal(got, want), (what, "corner stream of pass", p, gc.SHAPES[p], got.size, want.size)


def _same_range(e, c, what):
    """what the passes leave uncovered is what the quantiser codes"""
    for n in range(3):
        defs, nib, nn = c["census"]["range"][n]
        d2, n2, nn2 = e.range_streams(n)
        assert nn2 == nn and np.array_equal(d2, defs) and np.array_equal(n2, nib), (what, "range streams of plane", n, nn2, nn)


@pytest.mark.parametrize("name", gc.ALL_NAMES)
def test_against_the_oracle(hip_gen, oracle_built, name):
    c = gc.case(name)
    hip_gen.set_image(c["planes"])
    hip_gen.encode(c["rf"], False, False)
    _same_gradient(hip_gen, c, name)
    _same_range(hip_gen, c, name)


@pytest.mark.parametrize("names", gc.BATCHES, ids=["+".join(b) for b in gc.BATCHES])
def test_batch_of_three(hip, oracle_built, names):
    """the fused kernel's frame-strided form: three different frames of one shape, each compared with its own oracle run"""
    import torch
    cases = [gc.case(n) for n in names]
    frames = torch.from_numpy(np.ascontiguousarray(np.stack([c["planes"] for c in cases]))).cuda()
    hip.set_batch(frames)
    hip.encode_batch(cases[0]["rf"], False)
    for f, c in enumerate(cases):
        hip.select_frame(f)
        _same_gradient(hip, c, (names, "frame", f))
        _same_range(hip, c, (names, "frame", f))


@pytest.mark.parametrize("name", ["c_2", "g200x136"])
def test_graph_replay(hip, oracle_built, name):
    """encode_frame: the fused kernel inside the replayed graph; twice, so that the second is a replay"""
    c = gc.case(name)
    hip.set_image(c["planes"])
    for turn in range(2):
        hip.encode_frame(c["rf"], False)
        _same_gradient(hip, c, (name, "encode_frame", turn))
        _same_range(hip, c, (name, "encode_frame", turn))


@pytest.mark.parametrize("name", gc.C_NAMES)
def test_pixel_cache(hip, oracle_built, name):
    """the strips around the compact threshold with the pixel cache on: the fused kernel leaves the uncovered cells' pixels for the 1-D coder"""
    c = gc.case(name)
    opix, otyp = gc.oracle_1d(c["planes"], c["rf"])
    hip.set_pixel_cache(True)
    try:
        hip.set_image(c["planes"])
        hip.encode(c["rf"], False, False)
        _same_gradient(hip, c, (name, "pixel cache"))
        gpix, gtyp = hip.dynamic_tile_compressor()
        assert np.array_equal(gtyp, otyp), (name, "pixel cache", "1-D parameter stream", gtyp.size, otyp.size)
        assert np.array_equal(gpix, opix), (name, "pixel cache", "1-D pixel stream", gpix.size, opix.size)
    finally:
        hip.set_pixel_cache(False)
