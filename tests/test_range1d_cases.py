"""The directed 1-D range-coder inputs (tests/range1d_cases.py) are what they claim to be, shown from the reference alone: no GPU.

tests/test_gpu_range1d_directed.py rests on this file: every branch condition of yk_range1d_body / yk_dec1d_body it means to drive is asserted here
on the oracle's coverage and streams.  A failure here is a fault of the generator, not of a kernel."""
from collections import Counter

import numpy as np
import pytest

from tests import range1d_cases as rc


@pytest.fixture(scope="module")
def censuses(oracle_built):
    return {n: rc.census(rc.case(n)["planes"], rc.case(n)["per_plane"], rc.case(n)["run"]) for n in rc.ALL_NAMES}


@pytest.mark.parametrize("name", rc.ALL_NAMES)
def test_oracle_coverage_is_exactly_the_wanted_cells(oracle_built, name):
    c = rc.case(name)
    got, want = c["run"]["uncovered"], c["want"]
    for p in range(3):
        extra, missing = int((got[p] & ~want[p]).sum()), int((want[p] & ~got[p]).sum())
        assert (extra, missing) == (0, 0), (name, p, extra, missing)
    union = want[0] | want[1] | want[2]
    assert np.array_equal(c["run"]["shared"], union), "the all-plane map is the union of the planes' cells"
    if c["per_plane"]:
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])


def test_plug_image_forms():
    """the documented signature: [h/4, w/4] or [3, h/4, w/4], values on G / B only, int32 in 0..255, the deviation on the interior 3x3 alone"""
    want = np.zeros((4, 6), dtype=bool); want[1, 2] = True
    for bg in ("flat", "ramp"):
        base = rc.background(24, 16, bg)
        a = rc.plug_image(24, 16, want, {(1, 1, 2): range(9), (2, 1, 2): [255] * 9}, bg)
        assert a.dtype == np.int32 and a.shape == (3, 16, 24) and a.min() >= 0 and a.max() <= 255
        diff = a != base
        assert not diff[:, :, :8].any() and not diff[:, :4].any() and not diff[:, 4, :].any() and not diff[:, :, 8].any()
        assert np.array_equal(a[0, 5:8, 9:12], base[0, 5:8, 9:12] + rc.PLUG) and np.array_equal(a[1, 5:8, 9:12].ravel(), np.arange(9))
        b = rc.plug_image(24, 16, np.stack([want, ~want & False, want]), None, bg)
        assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], base[1]) and np.array_equal(b[2, 5:8, 9:12], base[2, 5:8, 9:12] + rc.PLUG)


def test_every_pattern_in_sparse_and_in_dense_strips(censuses):
    tiles = Counter()
    for n in rc.SHARED_NAMES:
        tiles.update(censuses[n]["tiles"])
    for pat in range(1, 16):
        assert tiles[(pat, "sparse")] > 0, ("no sparse strip holds pattern", pat)
        assert tiles[(pat, "dense")] > 0, ("no dense strip holds pattern", pat)


def test_every_pattern_in_every_plane_of_the_per_plane_cases(censuses):
    per = [Counter() for _ in range(3)]
    kinds = Counter()
    for n in rc.PER_PLANE_NAMES:
        assert censuses[n]["per_plane"] is not None
        for p in range(3):
            per[p].update(censuses[n]["per_plane"][p])
        kinds.update(censuses[n]["tiles"])
    for p in range(3):
        for pat in range(1, 16):
            assert per[p][pat] > 0, (p, pat)
    for pat in range(1, 16):                                               # the slot + pack form has both paths too
        assert kinds[(pat, "sparse")] > 0 and kinds[(pat, "dense")] > 0, pat


@pytest.mark.parametrize("names", [rc.SHARED_NAMES, rc.PER_PLANE_NAMES], ids=["shared", "per_plane"])
def test_strip_counts(censuses, names):
    counts = set()
    for n in names:
        counts |= censuses[n]["strip_counts"]
    assert {0, 1, 2, 3, 4, 5, 64} <= counts, sorted(counts)


def test_arrangements_of_the_sparse_strips(censuses):
    """four cells in four tiles, in the four macro-tiles of a strip, 2 + 2, 3 + 1 and one whole tile; and a first dense strip of five"""
    seen = set()
    for n in rc.SHARED_NAMES:
        want = rc.case(n)["want"][0]
        pats, sc = rc.tile_patterns(want), rc.strip_counts(want)
        for sy, bx in zip(*np.nonzero((sc == 4) | (sc == 5))):
            blk = pats[2 * sy: 2 * sy + 2, 8 * bx: 8 * bx + 8]
            sizes = sorted(bin(int(v)).count("1") for v in blk.ravel() if v)
            seen.add(tuple(sizes))
            if sizes == [1, 1, 1, 1] and blk.shape[1] == 8 and all(blk[:, 2 * m: 2 * m + 2].any() for m in range(4)):
                seen.add("macro")
    assert {(1, 1, 1, 1), "macro", (2, 2), (1, 3), (4,), (1, 4), (2, 3)} <= seen, seen


def test_value_regimes_reach_the_type_stream(censuses):
    """every regime, in a sparse and in a dense strip, with the triple worked out by hand in range1d_cases.REGIMES"""
    seen = set()
    for n in rc.SHARED_NAMES:
        rec = {(p, ty, tx): (kind, triple, pat) for p, ty, tx, pat, kind, triple, _ in censuses[n]["records"]}
        for p, ty, tx, regime, triple in rc.case(n)["expect"]:
            kind, got, pat = rec[(p, ty, tx)]
            assert got == triple, (n, regime, (p, ty, tx), pat, got, triple)
            seen.add((regime, kind))
    for regime in rc.REGIME_NAMES:
        assert (regime, "sparse") in seen and (regime, "dense") in seen, regime
    triples = set().union(*[censuses[n]["triples"] for n in rc.SHARED_NAMES])
    L = rc.FLAT
    assert {(1, L, 0), (254, L, 0), (L, 0, 0), (L + 50, L, 0), (L, L + 10, 1), (L, L + 10, 2), (L, L + 10, 3), (L, 0, 255), (L + 100, L, 60), (L, 40, 120)} <= triples
    assert any(t[0] == 220 for t in triples)                               # the three-way tie went to the right-most value


def test_value_regime_bytes(censuses):
    """the bytes each regime stands for: n = -1 codes as 0, the last index as 16, and one tile holds all 17"""
    found = Counter()
    for n in rc.SHARED_NAMES:
        c = rc.case(n)
        rec = {(p, ty, tx): (triple, b, pat) for p, ty, tx, pat, kind, triple, b in censuses[n]["records"]}
        for p, ty, tx, regime, _ in c["expect"]:
            triple, b, pat = rec[(p, ty, tx)]
            k = bin(pat).count("1")
            got = Counter(int(v) for v in b)
            if regime == "within1":
                assert set(got) == {0}
            elif regime in ("mode0", "mode255", "one_left"):
                assert got == {0: 9 * k, 1: 7 * k}                        # the background is the one value left: byte 1
            elif regime == "delta1":
                assert got == {0: 7 * k + (9 * k + 1) // 2, 15: 9 * k // 2}  # minCol itself: n = -1 -> 0
            elif regime == "delta2":
                assert got == {0: 7 * k, 1: 3 * k, 8: 3 * k, 16: 3 * k}
            elif regime == "delta255":
                assert got == {0: 7 * k, 1: (9 * k + 1) // 2, 16: 9 * k // 2}
            elif regime == "all17":
                assert set(got) == set(range(17))
            else:
                continue
            found[regime] += 1
    assert all(found[r] for r in ("within1", "mode0", "mode255", "one_left", "delta1", "delta2", "delta255", "all17")), found
    allbytes = set().union(*[censuses[n]["bytes"] for n in rc.SHARED_NAMES])
    assert allbytes >= set(range(17)) and max(allbytes) == 16


def test_edges(censuses):
    last_col = half_x = half_y = hi_sparse = hi_dense = 0
    for n in rc.ALL_NAMES:
        h, w = rc.case(n)["planes"].shape[1:]
        for p, ty, tx, pat, kind, triple, b in censuses[n]["records"]:
            last_col += w % 64 != 0 and tx * 8 >= w // 64 * 64
            half_x += w % 16 == 8 and tx * 8 >= w // 16 * 16
            half_y += h % 16 == 8 and ty * 8 >= h // 16 * 16
            if ty * (w // 8) + tx >= 1024:
                hi_sparse += kind == "sparse"
                hi_dense += kind == "dense"
    assert last_col and half_x and half_y and hi_sparse and hi_dense, (last_col, half_x, half_y, hi_sparse, hi_dense)


def test_full_scan_block(censuses):
    """the noise image: nothing covered, so the first scan block of 1024 tiles codes 1024 tiles and 65536 bytes per plane (the 11 + 21 bit packing's limit)"""
    c = rc.case(rc.NOISE)
    assert c["run"]["shared"].all() and c["run"]["uncovered"].all()
    recs = censuses[rc.NOISE]["records"]
    assert len(recs) == 3 * 33 * 33
    first = [r for r in recs if r[0] == 0 and r[1] * 33 + r[2] < 1024]
    assert len(first) == 1024 and all(r[3] == 15 for r in first) and sum(r[6].size for r in first) == 65536
    assert c["run"]["pix"].size == 3 * 1089 * 64 and c["run"]["type"].size == 3 * 1089 * 3


def test_batch_frames_differ():
    for names in rc.BATCHES.values():
        shapes = {rc.case(n)["planes"].shape for n in names}
        assert len(shapes) == 1 and len(names) == 3
        wants = [rc.case(n)["want"].tobytes() for n in names]
        assert len(set(wants)) == 3
