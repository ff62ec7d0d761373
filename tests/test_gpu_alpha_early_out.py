"""yk_alpha_kernel reads a tile in two steps: it probes the tile's first and last row, and only tiles in which the probe saw nothing have
their 14 rows in between read.  These cases put the deciding sample where each step, each guard and each lane mask has to find it.

Every comparison is against the CPU oracle's MipPrefilter (has_chunk, bounds, remaining, tile_bbox, bitmap, as tests/parity.py compares them).
The oracle's recursion is defined for square power-of-two images only.  For the other sizes the oracle runs on the same planes zero-padded to
the enclosing power-of-two square: padding adds rejected tiles only, so the box, the tile box, the bitmap over it and the remaining pixels
are those of the unpadded image -- except where the box is the whole (unpadded) image, the discard rule; cases about that rule are therefore
square powers of two.  compare_encode (the fused kernel's use of keep / bounds) needs the oracle's whole encode and runs the "every sample
position" pattern embedded in 512 x 512."""
import numpy as np
import pytest

from tests.parity import compare_encode
from yaik_amd import distributed as ykd

pytestmark = pytest.mark.gpu

ALPHA_KEYS = ("has_chunk", "bounds", "remaining", "tile_bbox", "bitmap")
UNPROBED_LAST = 14          # the last row of a tile that the probe does not read


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _noise_rgb(h, w, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (3, h, w)).astype(np.int32)


def _planes(alpha, rgb_noise=False):
    h, w = alpha.shape
    rgb = _noise_rgb(h, w) if rgb_noise else np.zeros((3, h, w), np.int32)
    return np.concatenate([rgb, alpha[None].astype(np.int32)])


def every_position(value, size=288, t0=1, drop=None):
    """size x size alpha; tile (t0 + i, t0 + j), i, j in 0..15, holds exactly one non-zero sample, at row i, column j of the tile.
    drop(i, j) -> True removes that tile's sample."""
    a = np.zeros((size, size), np.int32)
    for i in range(16):
        for j in range(16):
            if drop is None or not drop(i, j):
                a[(t0 + i) * 16 + i, (t0 + j) * 16 + j] = value
    return a


def _runs(i, j):
    """whole runs of 2, 8 and 16 tiles without a sample: row 3 tiles 4..5, row 6 tiles 8..15, row 9 every tile, row 12 tiles 0..7 and 14..15"""
    return (i == 3 and 4 <= j < 6) or (i == 6 and j >= 8) or i == 9 or (i == 12 and (j < 8 or j >= 14))


def probe_next_to_undecided(size=128):
    """opaque tiles interleaved (by tile, by pair of tiles and by row of tiles) with tiles whose only non-zero sample is in the last row the
    probe does not read; the outer ring of tiles stays empty"""
    a = np.zeros((size, size), np.int32)
    n = size // 16
    for ty in range(1, n - 1):
        for tx in range(1, n - 1):
            opaque = ((tx + ty) & 1) == 0 if ty < 3 else ((tx >> 1) & 1) == 0 if ty < 5 else (ty & 1) == 0
            if opaque:
                a[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = 255
            else:
                a[ty * 16 + UNPROBED_LAST, tx * 16 + (tx * 5 + ty) % 16] = 1 + (tx + ty) % 255
    return a


def wide_two_segments():
    """1040 x 48: a second, partial segment (16 pixels) and three rows of tiles (the second unit has a single row)"""
    a = np.zeros((48, 1040), np.int32)
    a[16 + 7, 3 * 16 + 2] = 9           # first segment, first unit, found by the second step
    a[32, 1039] = 200                   # second segment, second unit, found by the probe's first row
    a[32 + 9, 512 + 5] = 1              # first segment, second unit, second step
    return a


def last_column_and_row():
    """1048 x 40 (both sides 8 mod 16): the last tile column / row are kept by samples of the last image column / row alone"""
    a = np.zeros((40, 1048), np.int32)
    a[5, 1047] = 3                      # last image column, tile row 0
    a[39, 100] = 77                     # last image row = row 7 of the part tile: the row the probe's clamped last row reads
    a[38, 700] = 1                      # next to last image row: between the part tile's probed rows
    a[20, 20] = 5
    return a


def _cases():
    c = {}
    for v in (1, 255):
        c[f"every_position_{v}"] = every_position(v)
        c[f"checkerboard_{v}"] = every_position(v, drop=lambda i, j: (i + j) & 1 == 1)
        c[f"runs_{v}"] = every_position(v, drop=_runs)
    c["probe_next_to_undecided"] = probe_next_to_undecided()
    c["transparent"] = np.zeros((64, 64), np.int32)
    c["opaque"] = np.full((64, 64), 255, np.int32)
    c["wide_two_segments"] = wide_two_segments()
    c["last_column_and_row"] = last_column_and_row()
    one = np.zeros((16, 16), np.int32)
    one[8, 8] = 1
    c["one_tile_kept"] = one                                                               # box == image: the discard rule on one tile
    c["one_tile_empty"] = np.zeros((16, 16), np.int32)
    return c


CASES = _cases()


# ---- reference ------------------------------------------------------------------------------------------------------
def _pow2_square(h, w):
    return h == w and h >= 16 and (h & (h - 1)) == 0


def oracle_alpha(pyoracle, planes):
    n, h, w = planes.shape
    if _pow2_square(h, w):
        return pyoracle.OracleEncoder(planes).mip_prefilter()
    side = 16
    while side < max(h, w):
        side *= 2
    padded = np.zeros((n, side, side), np.int32)
    padded[:, :h, :w] = planes
    r = pyoracle.OracleEncoder(padded).mip_prefilter()
    assert tuple(int(v) for v in r["bounds"]) != (0, 0, w, h), "the discard rule needs a power-of-two square case"
    return r


_REF = {}


@pytest.fixture(scope="module")
def ref(oracle_built):
    """the oracle's result per case, computed once"""
    def get(name):
        if name not in _REF:
            _REF[name] = oracle_alpha(oracle_built, _planes(CASES[name]))
        return _REF[name]
    return get


def keep_grid(r, mth, mtw):
    """[mth, mtw] bool from an alpha result's tile box and bitmap"""
    g = np.zeros((mth, mtw), bool)
    if r["has_chunk"] and r["bounds"][2] > r["bounds"][0]:
        bx, by, tw, th = (int(v) for v in r["tile_bbox"])
        bits = np.unpackbits(np.asarray(r["bitmap"], np.uint8), bitorder="little")[:tw * th].reshape(th, tw).astype(bool)
        g[by:by + th, bx:bx + tw] = bits
    return g


def assert_same(got, want, what=""):
    for k in ALPHA_KEYS:
        if k in ("tile_bbox", "bitmap") and not want["has_chunk"]:
            continue
        assert np.array_equal(np.asarray(got[k]).ravel(), np.asarray(want[k]).ravel()), f"{what}{k}: {got[k]} vs {want[k]}"


@pytest.fixture(scope="module")
def enc():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


def fresh_result(planes):
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    try:
        e.set_image(planes)
        return e.mip_prefilter()
    finally:
        e.close()


# ---- tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_alpha_result_equals_oracle(ref, name):
    want = ref(name)
    got = fresh_result(_planes(CASES[name]))
    assert_same(got, want, name + " ")


def test_expected_values_are_not_trivial(ref):
    """what the cases claim about themselves, on the oracle's side"""
    for name, a in CASES.items():
        r, (h, w) = ref(name), a.shape
        box = tuple(int(v) for v in r["bounds"])
        if name in ("opaque", "one_tile_kept"):
            assert box == (0, 0, w, h) and not r["has_chunk"]
        elif name in ("transparent", "one_tile_empty"):
            assert box == (9999999, 9999999, -1, -1) and r["remaining"] == 0
        else:
            g = keep_grid(r, (h + 15) // 16, (w + 15) // 16)
            assert r["has_chunk"] and box != (0, 0, w, h) and g.any() and not g.all(), name
    g = keep_grid(ref("every_position_1"), 18, 18)
    assert g[1:17, 1:17].all() and g.sum() == 256
    g = keep_grid(ref("checkerboard_255"), 18, 18)
    assert g.sum() == 128 and g[1, 1] and not g[1, 2]


@pytest.mark.parametrize("value", [1, 255])
def test_every_position_whole_encode(oracle_built, enc, value):
    """the pattern of every_position in 512 x 512 (tiles 8..23), RGB noise under it: the fused kernel's use of keep / bounds"""
    planes = _planes(every_position(value, size=512, t0=8), rgb_noise=True)
    assert compare_encode(planes, enc, False) == []


def test_opaque_whole_encode(oracle_built, enc):
    """box == image: every reject is discarded"""
    planes = _planes(np.full((64, 64), 255, np.int32), rgb_noise=True)
    assert compare_encode(planes, enc, False) == []


def stripes_alpha():
    """128 x 128, two stripes of 64 rows: stripe 0's halo row (image row 64) holds a sample in a tile column that is empty in stripe 0"""
    a = np.zeros((128, 128), np.int32)
    a[64, 5 * 16 + 3] = 255             # row 0 of tile (4, 5): the halo row of stripe 0
    a[3 * 16 + UNPROBED_LAST, 2 * 16 + 1] = 1     # stripe 0, last tile row, second step
    a[16, 16] = 9                       # stripe 0, probe
    a[100, 100] = 4                     # stripe 1, second step
    return a


def test_stripes(oracle_built):
    from yaik_amd.encoder import HipTileEncoder
    a = stripes_alpha()
    planes = _planes(a)
    whole = oracle_built.OracleEncoder(planes).mip_prefilter()
    g = keep_grid(whole, 8, 8)
    assert g.sum() == 4 and g[4, 5] and not g[3, 5]
    encs, boxes = [], []
    try:
        for r in range(2):
            y0, h, halo = ykd.stripe_rows(128, 2, r)
            e = HipTileEncoder(0)
            encs.append(e)
            e.set_image(np.ascontiguousarray(planes[:, y0:y0 + h + halo, :]), full_h=128, y0=y0, halo_rows=halo)
            e.alpha_reject()
            boxes.append(e.stripe_bbox())
            ys, xs = np.nonzero(g[y0 // 16:(y0 + h) // 16])
            want = [xs.min() * 16, y0 + ys.min() * 16, xs.max() * 16 + 16, y0 + ys.max() * 16 + 16]
            assert boxes[-1].tolist() == want, (r, boxes[-1], want)
        gb = ykd.combine_bboxes(boxes)
        assert np.array_equal(gb, whole["bounds"])
        for r, e in enumerate(encs):
            y0, h, halo = ykd.stripe_rows(128, 2, r)
            e.alpha_finish(gb)
            ar = e.alpha_result()
            assert np.array_equal(ar["bounds"], whole["bounds"]) and np.array_equal(ar["tile_bbox"], whole["tile_bbox"])
            mine = np.zeros_like(g)
            mine[y0 // 16:(y0 + h) // 16] = g[y0 // 16:(y0 + h) // 16]            # the whole image's keep, this stripe's rows only
            assert np.array_equal(keep_grid({**ar, "has_chunk": True}, 8, 8), mine), r
            assert ar["remaining"] == 256 * int(mine.sum())
    finally:
        for e in encs:
            e.close()


def test_batch_equals_single_frames(oracle_built, enc):
    import torch
    alphas = [np.full((512, 512), 255, np.int32), np.zeros((512, 512), np.int32), every_position(1, size=512, t0=8)]
    host = [_planes(a, rgb_noise=True) for a in alphas]
    want = [oracle_built.OracleEncoder(p).mip_prefilter() for p in host]
    single = [fresh_result(p) for p in host]
    frames = torch.from_numpy(np.stack(host)).cuda()
    enc.set_batch(frames)
    for rep in range(2):                                    # the second run: arrival counters were left clean
        enc.encode_batch(3, False)
        for f in range(3):
            enc.select_frame(f)
            got = enc.alpha_result()
            assert_same(got, single[f], f"rep {rep} frame {f} vs single ")
            assert_same(got, want[f], f"rep {rep} frame {f} vs oracle ")


def test_handle_reuse(oracle_built):
    """one handle, opaque -> transparent -> sparse -> opaque: no stale decision, no stale arrival counter"""
    from yaik_amd.encoder import HipTileEncoder
    sparse = every_position(1, size=64, t0=0, drop=lambda i, j: i >= 4 or j >= 3)          # 64 x 64: tiles (0..3, 0..2)
    seq = [("opaque", CASES["opaque"]), ("transparent", CASES["transparent"]), ("sparse", sparse), ("opaque", CASES["opaque"])]
    e = HipTileEncoder(0)
    try:
        for step, (name, a) in enumerate(seq):
            planes = _planes(a)
            e.set_image(planes)
            got = e.mip_prefilter()
            assert_same(got, fresh_result(planes), f"step {step} {name} vs fresh handle ")
            assert_same(got, oracle_alpha(oracle_built, planes), f"step {step} {name} vs oracle ")
    finally:
        e.close()
