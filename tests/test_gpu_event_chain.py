"""The event chain of the encode entry points: yk_order_fused_after as one wait on the other handle's fused-end event (shared ownership of
that handle's event ring), kernel times with one record between the alpha kernel and the fused kernel, and the compaction kernels at the smallest shapes that reach each
of their branches.  Every result is compared with the oracle through tests/parity.py::compare_encode; the sequences under test queue their
own calls, so compare_encode is handed a view of the handle whose image and encode are already in place.

The oracle's MipPrefilter is defined for square power-of-two images only, so compare_encode cannot take an RGBA image of 320 x 256 or 328 x 264.
For those the oracle runs on the same planes zero-padded to the enclosing power-of-two square (as tests/test_gpu_alpha_early_out.py does):
padding adds rejected tiles only, so the box, the reject bitmap over it and -- the streams being row-major over the tile grid, and the box
ending 16 pixels inside the image -- the three planes' definition and nibble streams, which is what the compaction writes, are those of the
unpadded image.  The maps whose layout depends on the image's size (tile bitmaps, coverage) are compared on the RGB cases of these shapes and on
the square RGBA cases."""
import math

import numpy as np
import pytest

from oracle.pyoracle import PASSES, OracleEncoder
from tests.parity import compare_encode
from yaik_amd.synth import synth_planes

pytestmark = pytest.mark.gpu


class _Queued:
    """A handle whose encode has been queued by the test: compare_encode's set_image / mip_prefilter / encode do not run anything again."""

    def __init__(self, enc):
        self._e = enc

    def set_image(self, planes):
        pass

    def mip_prefilter(self):
        return self._e.alpha_result()

    def encode(self, *a, **k):
        pass

    def __getattr__(self, name):
        return getattr(self._e, name)


def _exact(planes, enc, mode3=False):
    n, h, w = planes.shape
    if n == 4 and not (h == w and h >= 16 and (h & (h - 1)) == 0):
        return _exact_padded(planes, enc, mode3)
    bad = compare_encode(planes, _Queued(enc), mode3, want_dst=False)
    assert not bad, bad


def _exact_padded(planes, enc, mode3):
    """RGBA, not a power-of-two square: the oracle on the zero-padded square (module docstring)"""
    n, h, w = planes.shape
    side = 16
    while side < max(h, w):
        side *= 2
    padded = np.zeros((n, side, side), np.int32)
    padded[:, :h, :w] = planes
    ora = OracleEncoder(padded)
    mo, mh = ora.mip_prefilter(), enc.alpha_result()
    assert tuple(int(v) for v in mo["bounds"]) != (0, 0, w, h), "the discard rule needs a power-of-two square case"
    for k in ("has_chunk", "bounds", "remaining", "tile_bbox", "bitmap"):
        assert np.array_equal(np.asarray(mh[k]), np.asarray(mo[k])), k
    for sx, sy in PASSES:                                     # the oracle's range pass codes what its gradient passes left uncovered
        ora.fitting_quad_smooth(sx, sy)
    for p in range(3):
        defs, nib, nn, _ = ora.dynamic_tile_encode(p, mode3)
        d2, n2, nn2 = enc.range_streams(p)
        assert nn2 == nn and nn > 0, (p, nn2, nn)
        assert np.array_equal(d2, defs) and np.array_equal(n2, nib), p


@pytest.fixture(scope="module")
def frames256():
    return [synth_planes(256, n_planes=4, seed=5100 + j) for j in range(2)]


@pytest.fixture
def pair():
    from yaik_amd.encoder import HipTileEncoder
    encs = [HipTileEncoder(0), HipTileEncoder(0)]
    yield encs
    for e in encs:
        e.close()


def _three_calls(e):
    e.alpha_reject(); e.alpha_finish(None); e.encode(3, False, False)


def test_ordered_both_directions_every_frame_exact(oracle_built, pair, frames256):
    """Two handles, 6 steps, order_fused_after in both directions, no host synchronisation in between; after the last step both handles hold a
    frame that equals the oracle's (every step rewrites all outputs from the same planes, so a step that ran out of order or early would show)."""
    for e, pl in zip(pair, frames256):
        e.set_image(pl)
    for step in range(6):
        for j, e in enumerate(pair):
            e.order_fused_after(pair[j - 1])
            _three_calls(e)
    for e, pl in zip(pair, frames256):
        _exact(pl, e)


@pytest.mark.parametrize("entry", ["frame", "batch"])
def test_ordered_through_the_other_entry_points(oracle_built, pair, frames256, entry):
    """The same sequence through yk_encode_frame (graph replay) and yk_encode_batch (a batch of 2 per handle)."""
    import torch
    if entry == "frame":
        for e, pl in zip(pair, frames256):
            e.set_image(pl)
    else:
        host = [[frames256[j], frames256[1 - j]] for j in range(2)]
        for e, fr in zip(pair, host):
            e.set_batch(torch.from_numpy(np.stack(fr)).cuda())
    for step in range(6):
        for j, e in enumerate(pair):
            e.order_fused_after(pair[j - 1])
            if entry == "frame":
                e.encode_frame(3, False)
            else:
                e.encode_batch(3, False)
    for j, e in enumerate(pair):
        if entry == "frame":
            _exact(frames256[j], e)
        else:
            for f in range(2):
                e.select_frame(f)
                _exact(host[j][f], e)


def test_other_handle_closed_before_the_ordered_encode(oracle_built, frames256):
    """a.order_fused_after(b), then b is destroyed, then a encodes: the event a waits on outlives b."""
    from yaik_amd.encoder import HipTileEncoder
    a, b = HipTileEncoder(0), HipTileEncoder(0)
    try:
        a.set_image(frames256[0]); b.set_image(frames256[1])
        _three_calls(b)
        a.order_fused_after(b)
        b.close()
        _three_calls(a)
        _exact(frames256[0], a)
        _three_calls(a)                                       # and the request was used up: nothing of b is touched again
        _exact(frames256[0], a)
    finally:
        a.close(); b.close()


def test_no_op_cases(oracle_built, pair, frames256):
    """Ordering behind a handle that has never encoded does nothing; two requests before one encode still give a correct encode."""
    a, b = pair
    a.set_image(frames256[0]); b.set_image(frames256[1])
    a.order_fused_after(b)                                    # b has never encoded
    _three_calls(a)
    _exact(frames256[0], a)
    _three_calls(b)
    a.order_fused_after(b); a.order_fused_after(b)
    _three_calls(a)
    _exact(frames256[0], a)
    _exact(frames256[1], b)


def _finite_nonneg(k):
    assert set(k) == {"encode", "alpha", "pack"}
    for name, v in k.items():
        assert math.isfinite(v) and v >= 0, (name, v)


@pytest.mark.parametrize("npl", [4, 3])
def test_timing_contract_after_a_short_run(oracle_built, pair, frames256, npl):
    """3 encodes, then kernel_ms(): finite values >= 0, encode > 0; an RGB frame has no alpha interval (0).  No absolute times."""
    e = pair[0]
    e.set_image(np.ascontiguousarray(frames256[0][:npl]))
    for _ in range(3):
        if npl == 4:
            e.alpha_reject(); e.alpha_finish(None)
        e.encode(3, False, False)
    k = e.kernel_ms()
    print(npl, k)
    _finite_nonneg(k)
    assert k["encode"] > 0
    if npl == 3:
        assert k["alpha"] == 0
    else:
        assert k["alpha"] > 0 and k["pack"] > 0


@pytest.mark.parametrize("entry", ["frame", "batch"])
def test_timing_contract_other_entry_points(oracle_built, pair, frames256, entry):
    import torch
    e = pair[0]
    if entry == "frame":
        e.set_image(frames256[0])
    else:
        e.set_batch(torch.from_numpy(np.stack(frames256)).cuda())
    for _ in range(3):
        e.encode_frame(3, False) if entry == "frame" else e.encode_batch(3, False)
    k = e.kernel_ms()
    print(entry, k)
    _finite_nonneg(k)
    assert k["encode"] > 0


def test_ring_wrap(oracle_built, pair, frames256):
    """70 encodes without a query (the 64-deep ring wraps, sets are recorded again while the handle is busy), then one kernel_ms()."""
    e = pair[0]
    e.set_image(frames256[0])
    for _ in range(70):
        _three_calls(e)
    k = e.kernel_ms()
    print(k)
    _finite_nonneg(k)
    assert k["encode"] > 0
    _exact(frames256[0], e)


def _boxed(w, h, npl, seed):
    """synthetic planes whose alpha box does not start at the origin (RGBA): kept tiles from (16, 16) up to 16 short of the far sides (64 x 64: up
    to the far sides), so that the fused kernel's `tgx + 8 <= cw` rule drops tiles inside the box"""
    p = synth_planes(w, h, n_planes=npl, seed=seed)
    rng = np.random.default_rng(seed)                          # noise in a third of the 4x4 cells: tiles of 0, 16, 32, 48 and 64 nibbles at every size
    cells = np.kron(rng.random(((h + 3) // 4, (w + 3) // 4)) < 0.35, np.ones((4, 4), bool))[:h, :w]
    p[:3] = np.where(cells[None], rng.integers(0, 256, (3, h, w)), p[:3]).astype(np.int32)
    if npl == 4:
        a = np.maximum(p[3], 1)
        keep = np.zeros_like(a)
        far = 0 if w <= 64 else 16                             # 64 x 64: the box runs to the far sides, or no tile would be left to code
        keep[16:(h - far) & ~15, 16:(w - far) & ~15] = 1
        p[3] = a * keep
    return p


@pytest.mark.parametrize("mode3", [False, True])
@pytest.mark.parametrize("npl", [3, 4])
@pytest.mark.parametrize("w,h", [(64, 64), (320, 256), (328, 264)])
def test_compaction_shapes(oracle_built, pair, w, h, npl, mode3):
    """64x64: one scan block; 320x256: 1280 tiles = two scan blocks on the run-sum path; 328x264: 41x33 tiles, a width that is no multiple of
    64, the scan2 path with two blocks."""
    e = pair[0]
    planes = _boxed(w, h, npl, 6200 + w)
    e.set_image(planes)
    if npl == 4:
        e.alpha_reject(); e.alpha_finish(None)
    e.encode(3, mode3, False)
    _exact(planes, e, mode3)


@pytest.mark.parametrize("mode3", [False, True])
@pytest.mark.parametrize("npl", [3, 4])
def test_compaction_batch_of_three(oracle_built, pair, npl, mode3):
    import torch
    e = pair[0]
    host = [_boxed(320, 256, npl, 6300 + f) for f in range(3)]
    e.set_batch(torch.from_numpy(np.stack(host)).cuda())
    e.encode_batch(3, mode3)
    for f in range(3):
        e.select_frame(f)
        _exact(host[f], e, mode3)
