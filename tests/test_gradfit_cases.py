"""The directed gradient-fit inputs (tests/gradfit_cases.py) are what they claim to be, shown from the reference alone: no GPU.

tests/test_gpu_gradfit_directed.py rests on this file: every branch condition of y2_grad_pass it means to drive (which variant keeps a tile, where
the others die, the strip's path, the curvature bound, the clamped corners) is asserted here on the oracle's accept / reject decisions and on the
numpy model of the six tests.  A failure here is a fault of the generator, not of a kernel."""
from collections import Counter, defaultdict

import numpy as np
import pytest

from tests import gradfit_cases as gc

V, SHAPES = gc.VARIANTS, gc.SHAPES


@pytest.fixture(scope="module")
def cases(oracle_built):
    return {n: gc.case(n) for n in gc.ALL_NAMES}


def _view(c, t):
    """(tile [3, TY, TX], corners as the reference reads them, x, y, TX, TY) of a target"""
    TX, TY = SHAPES[t["p"]]
    x, y = 4 * t["cx"], 4 * t["cy"]
    return c["planes"][:, y: y + TY, x: x + TX].astype(np.int64), gc.tile_corners(c["planes"], x, y, TX, TY), x, y, TX, TY


def _targets(cases, group):
    return [(c, t) for c in cases.values() for t in c["targets"] if t["group"] == group]


def test_model_by_hand():
    """variants() on a tile worked out by hand: corners 8, 8, 8, 8 except BR = 72: raw blends differ from Round6 (8 -> 8, 72 -> 73) at the far end"""
    corners = np.array([[8] * 3, [8] * 3, [8] * 3, [72] * 3])
    b = gc._blends(corners[None], 4, 4)[0]
    assert b[0, 0, 0, 0] == 8 and b[1, 0, 3, 3] == 8 + (64 * 9 + 8) // 16 and b[3, 0, 3, 3] == 8 + (65 * 9 + 8) // 16 and b[0, 0, 3, 3] == 8 + 64 * 9 // 16
    cur = b[1].copy()
    assert all(ok for ok, _ in gc.variants(cur, corners, 4, 4, 3).values())
    cur[2, 1, 3] += 4                                                     # channel 2, dx 3, dy 1: raw-R is 4 off there and nowhere else
    got = gc.variants(cur, corners, 4, 4, 3)
    assert got["raw-R"] == (False, (2, 3, 1)) and set(got) == set(V)
    assert gc.round6(191) == 190 and gc.round6p(191) == 195 and gc.round6p(255) == 255 and gc.round6(3) == 0


@pytest.mark.parametrize("name", gc.ALL_NAMES)
def test_model_agrees_with_the_oracle(cases, name):
    """for every viable tile of every pass: some variant survives in the model <=> the oracle accepted it; and the oracle accepted no tile that
    the kernel's viability rule (dead cells, top-left cell uncovered, inside the image) excludes"""
    cs = cases[name]["census"]
    assert cs["stray"] == []
    bad = [(k, r["survivors"], r["accepted"]) for k, r in cs["tiles"].items() if bool(r["survivors"]) != r["accepted"]]
    assert not bad, bad[:4]
    assert len(cs["tiles"]) > 0 and cases[name]["planes"].min() >= 0 and cases[name]["planes"].max() <= 255


@pytest.mark.parametrize("name", gc.ALL_NAMES)
def test_targets_hold_what_they_claim(cases, name):
    c = cases[name]
    cs, rf = c["census"], c["rf"]
    for t in c["targets"]:
        key = gc.target_tile(t)
        what = (name, t["group"], key, t["expect"])
        TX, TY = SHAPES[t["p"]]
        if t["expect"] == "dead":
            assert key not in cs["tiles"] and cs["dead"][t["cy"]: t["cy"] + TY // 4, t["cx"]: t["cx"] + TX // 4].any(), what
            continue
        assert key in cs["tiles"], what + ("not viable in its pass",)
        rec = cs["tiles"][key]
        if "path" in t:
            assert rec["path"] == t["path"], what + (rec["path"],)
        if t["expect"] == "sole":
            assert rec["survivors"] == (V[t["variant"]],) and rec["accepted"], what + (rec["survivors"],)
        elif t["expect"] == "accept":
            assert rec["accepted"] and rec["survivors"], what
        else:
            assert rec["survivors"] == () and not rec["accepted"] and rec["last"] is not None, what
        if t.get("decide"):
            cur, corners, _, _, _, _ = _view(c, t)
            ch, dx, dy, sign = t["decide"]
            ok, first, nf = gc._variants_many(cur[None], corners[None], TX, TY, rf)
            off = int(cur[ch, dy, dx] - gc._blends(corners[None], TX, TY)[0][t["variant"], ch, dy, dx])
            if t["expect"] == "sole":
                assert off == sign * rf, what
            else:                                                         # five dead anyway; the sixth fails in this pixel and in no other
                assert off == sign * (rf + 1) and nf[0, t["variant"]] == 1 and first[0, t["variant"]] == (dy * TX + dx) * 3 + ch, what
                cur[ch, dy, dx] -= sign
                assert gc._variants_many(cur[None], corners[None], TX, TY, rf)[0][0].tolist() == [i == t["variant"] for i in range(6)], what


def test_A_every_sole_survivor_class(cases):
    """from the census alone: (shape, variant, path) of every viable tile that exactly one variant keeps"""
    seen = Counter()
    for c in cases.values():
        if c["rf"] != 3:
            continue
        for (p, _, _), r in c["census"]["tiles"].items():
            if len(r["survivors"]) == 1 and r["accepted"]:
                seen[(SHAPES[p], r["survivors"][0], r["path"])] += 1
    want = [(SHAPES[p], v, path) for p in range(7) for v in V for path in gc.paths_of(p)]
    assert len(want) == 90 and len(gc.ABSENT) <= 8 and set(gc.ABSENT) <= set(want)
    for k in want:
        if k in gc.ABSENT:
            assert seen[k] == 0, ("listed as absent, yet present", k)
        else:
            assert seen[k] > 0, ("no sole survivor of this class", k)
    for p in range(7):
        for v in V:
            assert any(seen[(SHAPES[p], v, path)] for path in gc.paths_of(p)), (SHAPES[p], v)


def _pairs_complete(cases, group, factors, passes):
    """per (reject factor, shape, path, kind): accept and reject at pixels that between them hold every row, both end columns, the first and the
    last cell, both signs and the channels of the kind"""
    got = defaultdict(lambda: defaultdict(set))
    for c, t in _targets(cases, group):
        TX, TY = SHAPES[t["p"]]
        ch, dx, dy, sign = t["decide"]
        g = got[(c["rf"], t["p"], t["path"], t["kind"])]
        assert c["census"]["tiles"][gc.target_tile(t)]["path"] == t["path"]
        assert (dx, dy) != (0, 0) and (t["kind"] == "A") == (t["variant"] < 4)
        assert t["kind"] == "A" or (ch == 2) == (t["kind"] == "P4")       # stream 3 carries channels 0 | 1 of the Round6P corners, stream 4 channel 2
        for e in (t["expect"],):
            g[e] |= {("row", dy % 4), ("col", dx % 4), ("cell", (dx // 4 == 0 and dy // 4 == 0, dx // 4 == TX // 4 - 1 and dy // 4 == TY // 4 - 1)), ("sign", sign), ("ch", ch)}
    for rf in factors:
        for p in passes:
            TX, TY = SHAPES[p]
            for path in gc.paths_of(p):
                for kind, chans in (("A", (0, 1, 2)), ("P3", (0, 1)), ("P4", (2,))):
                    g = got[(rf, p, path, kind)]
                    for e in ("sole", "reject"):
                        need = {("row", r) for r in range(4)} | {("col", 0), ("col", 3), ("sign", 1), ("sign", -1)} | {("ch", n) for n in chans}
                        assert need <= g[e], (rf, SHAPES[p], path, kind, e, sorted(need - g[e]))
                        cells = {v for k, v in g[e] if k == "cell"}
                        assert any(f for f, _ in cells) and any(l for _, l in cells), (rf, SHAPES[p], path, kind, e, "first and last cell")


def test_B_deciding_pixels(cases):
    _pairs_complete(cases, "B", (3,), range(7))


def test_F_other_reject_factors(cases):
    assert gc.F_FACTORS == (0, 1, 64) and [SHAPES[p] for p in gc.F_PASSES] == [(16, 16), (8, 8), (4, 4)]
    _pairs_complete(cases, "F", gc.F_FACTORS, gc.F_PASSES)


def test_C_cell_counts(cases):
    """strips whose viable tiles hold exactly the wanted number of cells, on the path that count means, each with an accepted and a rejected
    target (16 cells of 16x16 are ONE tile: there the two strips of that count share the duty)"""
    by = defaultdict(list)
    for c, t in _targets(cases, "C"):
        by[(t["p"], t["count"])].append((c, t))
    seen = defaultdict(set)
    for (p, n), ts in by.items():
        kinds = set()
        for c, t in ts:
            cs = c["census"]
            r, col = t["strip"]
            path = "compact" if n <= gc.COMPACT_MAX_CELLS else ("smooth" if p == 0 and n == 64 else "screened")
            assert cs["paths"][(p, r, col)] == (path, n), (SHAPES[p], n, cs["paths"].get((p, r, col)))
            kinds.add(cs["tiles"][gc.target_tile(t)]["accepted"])
            seen[p].add(n)
        assert kinds == {True, False}, (SHAPES[p], n, kinds)
    assert {15, 16, 17, 64} <= seen[6] and {12, 16, 20, 64} <= seen[3] and {16, 32, 48, 64} <= seen[0]
    assert gc.COMPACT_MAX_CELLS == 16


def test_D_curvature_bound(cases):
    lim = gc.curvature_limit(3)
    assert lim == 13
    seen = set()
    for c, t in _targets(cases, "D"):
        if "curve" not in t:
            continue
        cur, _, _, _, TX, TY = _view(c, t)
        ch, triple, want = t["curve"]
        r = cur[:, ::4, :].reshape(3, TY // 4, TX // 4, 4)
        d2 = np.stack([np.abs(r[..., 0] - 2 * r[..., 1] + r[..., 2]), np.abs(r[..., 1] - 2 * r[..., 2] + r[..., 3])], -1)    # [3, cells y, cells x, triple]
        assert d2[ch, -1, -1, triple] == want == d2.max() and want == (lim if t["expect"] == "accept" else lim + 1), (c["name"], t["p"], t["curve"], int(d2.max()))
        assert c["census"]["dead"][t["cy"]: t["cy"] + TY // 4, t["cx"]: t["cx"] + TX // 4].any() == (t["expect"] == "dead")
        seen.add((t["p"], ch, triple, t["expect"]))
    assert seen == {(p, ch, tr, e) for p in range(7) for ch in range(3) for tr in (0, 1) for e in ("accept", "dead")}
    # a strip in which every cell is dead next to one in which exactly one cell is alive, and that one an accepted 4x4 tile
    ((c, t),) = [(c, t) for c, t in _targets(cases, "D") if t.get("lone")]
    dead = c["census"]["dead"]
    r, col = t["cy"] // 4, t["cx"] // 16
    assert col == 1 and dead[4 * r: 4 * r + 4, 0: 16].all() and dead[4 * r: 4 * r + 4, 32: 48].all()
    assert (~dead[4 * r: 4 * r + 4, 16: 32]).sum() == 1 and not dead[t["cy"], t["cx"]]
    assert c["census"]["paths"][(6, r, 1)] == ("compact", 1) and all((p, r, 0) not in c["census"]["paths"] for p in range(7))


def test_E_corner_values(cases):
    """every value and every mixed triple is the TL of a viable 8x8 target; where a Round6P variant can keep such a tile it is its sole
    survivor, where it cannot (it moves TL itself by more than rf) the target is a reject; the saturated differences are rejects too"""
    c = cases["e_0"]
    got = defaultdict(set)
    sat = set()
    for t in c["targets"]:
        rec = c["census"]["tiles"][gc.target_tile(t)]
        cur, corners, *_ = _view(c, t)
        if "sat" in t:
            assert rec["survivors"] == () and set(np.unique(corners)) == {t["sat"][0]} and sorted(np.unique(cur)) == sorted(t["sat"]) and (cur == t["sat"][1]).sum() == 1
            sat.add((t["sat"], rec["path"]))
            continue
        assert tuple(int(v) for v in corners[0]) == t["tl"]
        got[t["tl"]].add((t["expect"], V[t["variant"]]) if t["expect"] == "sole" else ("reject",))
        moved = np.abs(gc.round6p(corners[0]) - corners[0]).max()
        if moved > 3:                                                     # Round6P's own TL is off by more than rf: it can never keep the tile
            assert t["expect"] == "reject", t["tl"]
    assert set(got) == {(v, v, v) for v in gc.E_VALUES} | set(gc.E_TRIPLES)
    assert got[(191, 191, 191)] == {("reject",)}
    sole = {tl for tl, g in got.items() if any(e[0] == "sole" for e in g)}
    # worked out, not observed: Round6P moves 191 -> 195, four off; every other listed value moves by at most 3 (127 -> 130, 63 -> 65, 255 -> 255)
    for v in gc.E_VALUES:
        if abs(int(gc.round6p(v)) - v) <= 3:
            assert (v, v, v) in sole, ("no Round6P sole survivor at", v, dict(got))
    assert {(255, 127, 255), (127, 255, 128)} <= sole, dict(got)
    assert {s for s, _ in sat} == {(255, 0), (0, 255)} and {p for _, p in sat} == {"compact", "screened"}


def test_H_window_edges(cases):
    """16x16 tiles, every variant, every path: D = S' - 256 cur of the deciding pixel sits on each end of the variant's window in an accepted
    tile and one beyond it in a rejected one (the bounds follow from blend-O = S' >> 8, blend-R = (S' + 127) >> 8 and |cur - blend| <= rf)"""
    seen = set()
    for c, t in _targets(cases, "H"):
        cur, corners, _, _, TX, TY = _view(c, t)
        ch, dx, dy, sign = t["decide"]
        rf, v = c["rf"], t["variant"]
        sp = int(gc.s_prime(corners, TX, TY)[v // 2][ch, dy, dx])
        D = sp - 256 * int(cur[ch, dy, dx])
        lo, hi = (-256 * rf, 256 * rf + 255) if v % 2 == 0 else (-256 * rf - 127, 256 * rf + 128)
        assert (TX, TY) == (16, 16) and sp % 256 == t["frac"]
        want = {(1, "sole"): lo, (1, "reject"): lo - 1, (-1, "sole"): hi, (-1, "reject"): hi + 1}[(sign, t["expect"])]
        assert D == want, (c["name"], V[v], t["frac"], sign, t["expect"], D, want)
        seen.add((c["census"]["tiles"][gc.target_tile(t)]["path"], v, sign, t["expect"]))
    assert seen == {(path, v, s, e) for path in gc.paths_of(0) for v in range(6) for s in (1, -1) for e in ("sole", "reject")}


def test_G_image_edges(cases):
    assert gc.G_SIZES == ((72, 24), (136, 40), (200, 136))
    edges, shapes = Counter(), set()
    for w, h in gc.G_SIZES:
        c = cases[f"g{w}x{h}"]
        planes = c["planes"]
        flat = planes.reshape(3, -1)
        assert planes.shape == (3, h, w) and w % 16 == 8 and h % 16 == 8
        dead = c["census"]["dead"]
        assert dead[:, (w + 15) // 16 * 4:].all() and dead.shape[1] > (w + 15) // 16 * 4                  # macro-tiles whose origin is outside
        for t in c["targets"]:
            cur, corners, x, y, TX, TY = _view(c, t)
            assert c["census"]["tiles"][gc.target_tile(t)]["accepted"], (w, h, t)
            beyond = [(cx_, cy_) for cy_ in (y, y + TY) for cx_ in (x, x + TX)]
            clamped = [k for k, (cx_, cy_) in enumerate(beyond) if cx_ >= w or cy_ >= h]
            assert clamped and (x + TX == w or y + TY == h) and (x + 2 * TX > w or y + 2 * TY > h), (w, h, t)
            assert (t["edge"] == "corner") == (len(clamped) == 3)
            # acceptance depends on the clamp: a zero, or what a read that runs on into the next row finds, rejects the tile
            for k in clamped:
                cx_, cy_ = beyond[k]
                wrong = [np.zeros(3, np.int64)]
                if cy_ * w + cx_ < w * h:
                    wrong.append(flat[:, cy_ * w + cx_].astype(np.int64))
                for v in wrong:
                    other = corners.copy()
                    other[k] = v
                    assert np.abs(v - corners[k]).max() > 60
                    assert not gc._variants_many(cur[None], other[None], TX, TY, 3)[0].any(), (w, h, t, k, v)
            edges[t["edge"]] += 1
            shapes.add((t["edge"], TX, TY))
        # a tile that does not fit next to one that just fits: the 16-wide tile at the last macro-tile column, the 8-wide one there
        keys = set(c["census"]["tiles"])
        assert not any(p in (0, 1) and tx * 16 + 16 > w for p, _, tx in keys) and any(p in (2, 3, 4) and tx * 8 + 8 == w for p, _, tx in keys)
        assert not any(p in (0, 2) and ty * 16 + 16 > h for p, ty, _ in keys) and any(p in (1, 3, 5) and ty * 8 + 8 == h for p, ty, _ in keys)
    assert edges["right"] >= 5 and edges["bottom"] >= 5 and edges["corner"] == 3
    assert {(e, tx, ty) for e, tx, ty in shapes if e == "right"} >= {("right", 8, 16), ("right", 8, 8), ("right", 8, 4), ("right", 4, 8), ("right", 4, 4)}
    assert {(e, tx, ty) for e, tx, ty in shapes if e == "bottom"} >= {("bottom", 16, 8), ("bottom", 8, 8), ("bottom", 4, 8), ("bottom", 8, 4), ("bottom", 4, 4)}


def test_batches_hold_three_different_frames_of_one_shape(cases):
    used = set()
    for names in gc.BATCHES:
        frames = [gc.case(n) for n in names]
        assert len(names) == 3 and len({f["planes"].shape for f in frames}) == 1 and len({f["rf"] for f in frames}) == 1
        assert len({f["planes"].tobytes() for f in frames}) == 3
        used |= set(names)
    assert used >= set(gc.ALL_NAMES)
