"""The grouped compact sweep of the fused encode kernel (y2_grad_pass in yk_encode2.hip: a compact pass from 8x8 on evaluates the next pass in the
same sweep when the two fit 16 cells) against the CPU oracle, bit for bit, on strips built tile by tile (tests/compact_group_cases.py;
tests/test_compact_group_cases.py shows from the oracle alone what every strip holds): cell counts on and just beyond the fit, both passes
rejecting, either one accepting, a first-pass tile that covers the origin of a second-pass tile that would be accepted, one that overlaps it without
covering the origin, one pass lost in stage 1 while the other is decided in stage 2, tiles of both passes on one origin lane with different fates,
reject factors 0 and 64, and strips on the right edge of images 72 and 136 wide.  Kernel version 2 (the product library), single images and
batches of three."""
import numpy as np
import pytest

from tests import compact_group_cases as q
from tests import gradfit_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from tests.parity import encoder_for_kernel_version
    e = encoder_for_kernel_version(2)
    yield e
    e.close()


def _same_as_census(e, c, what):
    cs = c["census"]
    h, w = c["planes"].shape[1:]
    for p in range(7):
        bm = cs["grad"][p][1]
        got = e.gradient_bitmap(p)
        assert got.size == bm.size, (what, "bitmap size of pass", p)
        if not np.array_equal(got, bm):
            a, b = gc.bitmap_tiles(got, p, w, h), gc.bitmap_tiles(bm, p, w, h)
            bad = [(int(ty), int(tx), "kernel accepts" if a[ty, tx] else "kernel rejects") for ty, tx in np.argwhere(a != b)]
            strips = [(col, s.name, s.own, s.spec) for col, s in c["strips"]]
            raise AssertionError((what, "pass", p, gc.SHAPES[p], "tiles (ty, tx) that differ", bad[:6], "strips", strips))
    assert e.gradient_counts().tolist() == [g[0] for g in cs["grad"]], (what, "counts")
    assert np.array_equal(e.coverage(), cs["coverage"]), (what, "coverage")
    for n in range(3):
        defs, nib, nn = cs["range"][n]
        d2, n2, nn2 = e.range_streams(n)
        assert nn2 == nn and np.array_equal(d2, defs) and np.array_equal(n2, nib), (what, "range streams of plane", n)


@pytest.mark.parametrize("name", q.NAMES)
def test_single_image(hip, oracle_built, name):
    from tests.parity import compare_encode
    c = q.case(name)
    if c["rf"] == 3:                                                       # compare_encode runs both sides at the default reject factor
        assert compare_encode(c["planes"], hip, mode3bit_only=False, want_dst=False, check_corners=True) == [], name
    hip.set_image(c["planes"])
    hip.encode(c["rf"], False, False)
    _same_as_census(hip, c, name)


@pytest.mark.parametrize("names", q.BATCHES, ids=[b[0] for b in q.BATCHES])
def test_batch_of_three(hip, oracle_built, names):
    import torch
    cases = [q.case(n) for n in names]
    hip.set_batch(torch.from_numpy(np.ascontiguousarray(np.stack([c["planes"] for c in cases]))).cuda())
    hip.encode_batch(cases[0]["rf"], False)
    for f, c in enumerate(cases):
        hip.select_frame(f)
        _same_as_census(hip, c, (names, "frame", f))
