"""yk_alpha_kernel as one-wave streaming units, the image-wide box folded by yk_alpha_box_kernel behind it.  A unit is 16 tile columns (a
256-pixel segment) times R rows of tiles; it leaves its box in a slot of its own and the fold is the only place where the image's box exists.
These cases are the smallest shapes that reach each edge of that split: units that are mostly outside the image, a last column segment of
half a tile, a last unit with fewer than R rows of tiles, a last row of tiles cut at 8, a box that spans units in both directions, units in
which the second step runs for some rows of tiles only, slots left over from the previous frame, frames of a batch, a stripe's y0.

R is a build parameter of the library (YK_ALPHA_R, 4 or 8): every shape that depends on it is run for both values.

Every comparison is against the CPU oracle's MipPrefilter on the keys has_chunk, bounds, remaining, tile_bbox, bitmap (as tests/parity.py
compares them); sizes that are no power-of-two square run the oracle on the zero-padded enclosing square, as tests/test_gpu_alpha_early_out.py
does (its helpers are used here), and the cases about the whole-image discard rule are square powers of two."""
import numpy as np
import pytest

from tests.parity import compare_encode
from tests.test_gpu_alpha_early_out import _planes, assert_same, fresh_result, keep_grid, oracle_alpha
from yaik_amd import distributed as ykd

pytestmark = pytest.mark.gpu

RS = (4, 8)                 # the values YK_ALPHA_R may take
EMPTY = (9999999, 9999999, -1, -1)
UNPROBED = 14               # a row of a tile that the probe does not read


def _zeros(w, h):
    return np.zeros((h, w), np.int32)


def single_16():
    a = _zeros(16, 16)
    a[9, 6] = 1
    return a


def half_tile_264x136():
    """264 x 136: the second column segment holds half a tile, the last row of tiles is cut at 8 (R = 4: the last unit has one row of tiles)"""
    a = _zeros(264, 136)
    a[70, 263] = 5              # the half tile, found by the second step
    a[135, 40] = 9              # the image's last row: the part tile's clamped probe row
    a[134, 200] = 1             # between the part tile's probed rows
    a[16, 16] = 200             # probe, first segment
    return a


def half_tile_520(R):
    """520 x (16 R + 8): three column segments, the last one half a tile; the second row of units is one row of tiles cut at 8"""
    h = 16 * R + 8
    a = _zeros(520, h)
    a[h - 1, 519] = 3           # last column, last row
    a[h - 2, 300] = 1           # the part tile's rows between its probed rows, second segment
    a[16 * (R - 1) + UNPROBED, 512 + 5] = 7     # the half tile of the first unit's last row of tiles
    a[5, 17] = 255
    return a


def four_corners(R, margin=0):
    """(256 + 16) x (16 R + 16): one sample in each corner tile, so the box spans units in both directions and exists only after the fold.
    The box is the whole image, which the padded oracle cannot tell from a larger one: test_four_corners compares what it can, and the same
    samples with `margin` empty pixels along the right and the bottom (box != image) go through the full comparison."""
    w, h = 272, 16 * R + 16
    a = _zeros(w + margin, h + margin)
    a[0, 0] = 1                 # probe row 0
    a[7, w - 3] = 2             # second step
    a[h - 1, 9] = 3             # probe row 15
    a[h - 16 + UNPROBED, w - 16] = 4
    return a


def some_rows_undecided(R):
    """272 x 32 R: tiles of column segment 0 kept by a sample in row 14 alone, in rows of tiles 0, R - 1 and R.  Rows of tiles 1 and R + 1 are
    opaque over the whole width (decided by the probe: the second step skips them), every other tile is empty (undecided, read, rejected):
    at R = 4 the first unit reads the rows of tiles 0 and 2 together and then row 3 on its own."""
    w, h = 272, 32 * R
    a = _zeros(w, h)
    for k, ty in enumerate((0, R - 1, R)):
        a[ty * 16 + UNPROBED, (3 + 4 * k) * 16 + k] = 1 + k
    a[16:32, :] = 255
    a[(R + 1) * 16:(R + 2) * 16, :] = 255
    return a


def _cases():
    c = {"single_16": single_16(), "half_tile_264x136": half_tile_264x136(), "transparent_272x144": _zeros(272, 144),
         "opaque_256": np.full((256, 256), 255, np.int32)}
    for R in RS:
        c[f"half_tile_520_R{R}"] = half_tile_520(R)
        c[f"four_corners_in_margin_R{R}"] = four_corners(R, margin=16)
        c[f"some_rows_undecided_R{R}"] = some_rows_undecided(R)
    return c


CASES = _cases()
_REF = {}


@pytest.fixture(scope="module")
def ref(oracle_built):
    """the oracle's result per plane, computed once per key"""
    def get(key, alpha=None):
        if key not in _REF:
            _REF[key] = oracle_alpha(oracle_built, _planes(CASES[key] if alpha is None else alpha))
        return _REF[key]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_alpha_result_equals_oracle(ref, name):
    assert_same(fresh_result(_planes(CASES[name])), ref(name), name + " ")


def test_expected_values_are_not_trivial(ref):
    """what the cases claim about themselves, on the oracle's side"""
    for name in ("single_16", "opaque_256"):
        h, w = CASES[name].shape
        assert tuple(int(v) for v in ref(name)["bounds"]) == (0, 0, w, h) and not ref(name)["has_chunk"]
    r = ref("transparent_272x144")
    assert tuple(int(v) for v in r["bounds"]) == EMPTY and r["remaining"] == 0      # (the oracle still reports a chunk: only box == image drops it)
    assert ref("half_tile_264x136")["bounds"].tolist() == [16, 16, 272, 144]          # the box is in whole tiles, past the cut sides
    for R in RS:
        w, h = 272, 16 * R + 16
        r = ref(f"four_corners_in_margin_R{R}")
        assert r["bounds"].tolist() == [0, 0, w, h] and r["has_chunk"] and keep_grid(r, h // 16 + 1, w // 16 + 1).sum() == 4
        r = ref(f"half_tile_520_R{R}")
        assert r["bounds"].tolist() == [16, 0, 528, 16 * R + 16]
        g = keep_grid(r, R + 1, 33)
        assert g.sum() == 4 and g[R, 32] and g[R - 1, 32] and g[R, 18] and g[0, 1]
        g = keep_grid(ref(f"some_rows_undecided_R{R}"), 2 * R, 17)
        assert g.sum() == 3 + 2 * 17 and g[0, 3] and g[R - 1, 7] and g[R, 11] and g[1].all() and g[R + 1].all()


@pytest.mark.parametrize("R", RS)
def test_four_corners(oracle_built, R):
    """the box is the whole (unpadded) image: the oracle on the padded square gives the box, the discard rule (bbox == image: every reject
    discarded, no chunk) gives the rest"""
    a = four_corners(R)
    h, w = a.shape
    padded = np.zeros((4, 512, 512), np.int32)
    padded[3, :h, :w] = a
    want = oracle_built.OracleEncoder(padded).mip_prefilter()
    assert want["bounds"].tolist() == [0, 0, w, h] and keep_grid(want, 32, 32).sum() == 4
    got = fresh_result(_planes(a))
    assert got["bounds"].tolist() == want["bounds"].tolist()
    assert not got["has_chunk"] and got["remaining"] == w * h


def test_opaque_whole_encode(oracle_built):
    """box == image after the fold: every reject is discarded by the fused kernel"""
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    try:
        assert compare_encode(_planes(CASES["opaque_256"], rgb_noise=True), e, False) == []
    finally:
        e.close()


def test_stale_slots(ref):
    """one handle: opaque, one sample, all zero, then a smaller image.  Every unit slot is rewritten by every launch, so each matches a fresh handle."""
    from yaik_amd.encoder import HipTileEncoder
    one = _zeros(256, 256)
    one[200 + 0, 130] = 1
    seq = [("opaque_256", CASES["opaque_256"]), ("one_sample_256", one), ("transparent_256", _zeros(256, 256)),
           ("half_tile_264x136", CASES["half_tile_264x136"])]
    e = HipTileEncoder(0)
    try:
        for step, (name, a) in enumerate(seq):
            planes = _planes(a)
            e.set_image(planes)
            got = e.mip_prefilter()
            assert_same(got, fresh_result(planes), f"step {step} {name} vs fresh handle ")
            assert_same(got, ref(name, a), f"step {step} {name} vs oracle ")
    finally:
        e.close()


def test_batch_equals_single_frames(ref):
    """three 272 x 144 frames with different boxes: each frame's units and fold use the frame's own slots"""
    import torch
    from yaik_amd.encoder import HipTileEncoder
    alphas = [_zeros(272, 144) for _ in range(3)]
    alphas[0][3, 260] = 1                                   # second segment only
    alphas[1][100:144, 30:90] = 255                         # the lower units of the first segment
    alphas[2][16 * 4 + UNPROBED, 16 * 16 + 1] = 9           # second step, second segment
    alphas[2][20, 20] = 1
    host = [_planes(a, rgb_noise=True) for a in alphas]
    want = [ref(f"batch_frame_{f}", a) for f, a in enumerate(alphas)]
    assert len({tuple(int(v) for v in r["bounds"]) for r in want}) == 3
    single = [fresh_result(p) for p in host]
    e = HipTileEncoder(0)
    try:
        e.set_batch(torch.from_numpy(np.stack(host)).cuda())
        for rep in range(2):
            e.encode_batch(3, False)
            for f in range(3):
                e.select_frame(f)
                got = e.alpha_result()
                assert_same(got, single[f], f"rep {rep} frame {f} vs single ")
                assert_same(got, want[f], f"rep {rep} frame {f} vs oracle ")
    finally:
        e.close()


def test_stripe_with_y0_and_halo(ref):
    """272 x 384 in three stripes of 128 rows: the middle one has y0 = 128 and a halo row.  Its box is that of the whole image's rows
    128..255 (in image coordinates), the halo row's sample belongs to the next stripe."""
    from yaik_amd.encoder import HipTileEncoder
    a = _zeros(272, 384)
    a[256, 5 * 16 + 3] = 255                                # the middle stripe's halo row, a tile column that is empty in the stripe
    a[128 + 16 + UNPROBED, 16 * 16 + 2] = 1                 # middle stripe, second segment, second step
    a[128 + 100, 40] = 7                                    # middle stripe, a later row of tiles (another unit at R = 4)
    a[10, 10] = 3                                           # first stripe
    planes = _planes(a)
    g = keep_grid(ref("stripes_272x384", a), 24, 17)
    assert g.sum() == 4 and g[16, 5] and g[9, 16] and g[14, 2]
    y0, h, halo = ykd.stripe_rows(384, 3, 1)
    assert (y0, h, halo) == (128, 128, 1)
    e = HipTileEncoder(0)
    try:
        e.set_image(np.ascontiguousarray(planes[:, y0:y0 + h + halo, :]), full_h=384, y0=y0, halo_rows=halo)
        e.alpha_reject()
        ys, xs = np.nonzero(g[y0 // 16:(y0 + h) // 16])
        want = [xs.min() * 16, y0 + ys.min() * 16, xs.max() * 16 + 16, y0 + ys.max() * 16 + 16]
        assert want == [32, 144, 272, 240]
        assert e.stripe_bbox().tolist() == want
    finally:
        e.close()
