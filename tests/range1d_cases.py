"""TEST INFRASTRUCTURE ONLY.  Directed inputs for the live 1-D range path (DynamicTileCompressor, the '1DTL' chunk) and its decoder.

The control flow of yk_range1d_body / yk_dec1d_body depends on WHICH 4x4 cells of an image the gradient passes leave uncovered.  plug_image() sets
that exactly, without a hook in the library: on a background the gradient tiles fit exactly (flat, or a ramp that is linear inside every 16x16
block), +60 on the interior 3x3 pixels (rows 1..3, columns 1..3) of a 4x4 cell of plane R makes every tile over that cell fail and touches no
sample of a neighbouring cell's fit (those read this cell's first row and column only).  Coverage is shared by the planes, so R decides it and
the interior 3x3 of G and B is free to carry the value regimes of the coder (mode clamps, delta 0 .. 255, ties, every byte 0..16).

layout() places the cells per 64x16 strip (one workgroup of the coder): strips with 1..4 uncovered cells (the coder's sparse path) in every
arrangement over tiles and macro-tiles, strips with 5 (the first count of the dense path), dense strips holding every quadrant pattern 1..15, full
strips and empty ones.  census() reads back, from the oracle's outputs alone, what a case really holds; tests/test_range1d_cases.py asserts on it.

A tile's quadrant pattern: bit 0 = top-left 4x4 cell uncovered, bit 1 = top-right, bit 2 = bottom-left, bit 3 = bottom-right.
"""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np

from oracle.pyoracle import PASSES, OracleEncoder
from tests.blobs import PP_MASKS

PLUG = 60            # far over the reject factor (3) of every pass
FLAT = 100           # level of the flat background


# ---- images ------------------------------------------------------------------------------------------------------------------------------------
def _tri(n: int) -> np.ndarray:
    """0..16..0 with its kinks at multiples of 16: linear inside every 16-aligned block, so inside every gradient tile of every pass"""
    t = np.arange(n) % 32
    return 16 - np.abs(t - 16)


def background(w: int, h: int, bg: str) -> np.ndarray:
    """int32 [3, h, w].  "flat": every plane FLAT.  "ramp": R = 64 + tri(x) + tri(y), G = 40 + 2 tri(x), B = 30 + tri(x) + 2 tri(y): bilinear with
    integer corner values inside every 16x16 block, slopes of at most 3 per pixel (the reference clamps the corner samples of the last tile
    column / row to the image, which bends the fit there by less than one slope: under the reject factor)."""
    if bg == "flat":
        return np.full((3, h, w), FLAT, dtype=np.int32)
    if bg != "ramp":
        raise ValueError(bg)
    tx, ty = _tri(w)[None, :], _tri(h)[:, None]
    return np.stack([64 + tx + ty, 40 + 2 * tx + 0 * ty, 30 + tx + 2 * ty]).astype(np.int32)


def plug_image(w: int, h: int, want: np.ndarray, values=None, bg: str = "ramp") -> np.ndarray:
    """int32 planes [3, h, w] whose gradient coverage leaves exactly the cells of `want` uncovered.  want: bool [3, h/4, w/4] (per plane, for the
    plane-subset passes) or [h/4, w/4] (shared coverage, driven by R alone).  values: {(plane 1 | 2, cell y, cell x): 9 values}, the interior 3x3
    of G / B in that cell, row-major."""
    want = np.asarray(want, dtype=bool)
    planes = background(w, h, bg)
    per_plane = want.ndim == 3
    assert want.shape[-2:] == (h // 4, w // 4), (want.shape, w, h)
    for p in range(3 if per_plane else 1):
        for cy, cx in zip(*np.nonzero(want[p] if per_plane else want)):
            planes[p, 4 * cy + 1: 4 * cy + 4, 4 * cx + 1: 4 * cx + 4] += PLUG
    for (p, cy, cx), v in (values or {}).items():
        assert p in (1, 2) and not per_plane
        planes[p, 4 * cy + 1: 4 * cy + 4, 4 * cx + 1: 4 * cx + 4] = np.asarray(v, dtype=np.int32).reshape(3, 3)
    return np.clip(planes, 0, 255).astype(np.int32)


# ---- layouts: which cells of which strip ----------------------------------------------------------------------------------------------------------
ONE, TWO, THREE = (1, 2, 4, 8), (3, 5, 6, 9, 10, 12), (7, 11, 13, 14)
RECIPES = ("s1", "s2_tiles", "s2_tile", "s3_tiles", "s3_tile", "s4_tiles", "s4_macro", "s4_2+2", "s4_3+1", "s4_15", "five", "denseA", "denseB", "full", "empty", "seven")


def _strip_patterns(recipe: str, r: int, ntx: int, nty: int) -> dict:
    """{(tile y, tile x) inside the strip: pattern} for a strip of ntx x nty tiles; r rotates the choice of tiles and patterns"""
    tiles = [(ty, tx) for ty in range(nty) for tx in range(ntx)]
    nt = len(tiles)

    def spread(k, step=3):
        """k different tiles, as far as the strip has them"""
        out, i = [], (r * 5) % nt
        while len(out) < min(k, nt):
            if tiles[i % nt] not in out:
                out.append(tiles[i % nt]); i += step
            else:
                i += 1
        return out

    one, two, three = (lambda i: ONE[(r + i) % 4]), (lambda i: TWO[(r + i) % 6]), (lambda i: THREE[(r + i) % 4])
    if recipe == "s1":
        return {spread(1)[0]: one(0)}
    if recipe == "s2_tiles":
        return {t: one(i) for i, t in enumerate(spread(2))}
    if recipe == "s2_tile":
        return {spread(1)[0]: two(0)}
    if recipe == "s3_tiles":
        return {t: one(i) for i, t in enumerate(spread(3))}
    if recipe == "s3_tile":
        return {spread(1)[0]: three(0)}
    if recipe == "s4_tiles":
        return {t: one(i) for i, t in enumerate(spread(4))}
    if recipe == "s4_macro":                                               # one cell in each of the strip's four 16x16 macro-tiles
        if ntx < 8:
            return {t: one(i) for i, t in enumerate(spread(4))}
        return {((r + m) % nty, 2 * m + ((r + m) >> 1) % 2): one(m) for m in range(4)}
    if recipe == "s4_2+2":
        return {t: two(3 * i) for i, t in enumerate(spread(2))} if nt > 1 else {tiles[0]: 15}
    if recipe == "s4_3+1":
        return {t: (three(0) if i == 0 else one(1)) for i, t in enumerate(spread(2))} if nt > 1 else {tiles[0]: 15}
    if recipe == "s4_15":
        return {spread(1)[0]: 15}
    if recipe == "five":                                                   # the first dense count: 4 + 1, or 3 + 2
        if nt == 1:
            return {tiles[0]: 15}
        a, b = spread(2)
        return {a: 15, b: one(0)} if r % 2 == 0 else {a: three(0), b: two(0)}
    if recipe == "denseA":                                                 # patterns 1..8 with covered tiles in between
        return {tiles[(2 * i + r) % nt]: i + 1 for i in range(min(8, (nt + 1) // 2))}
    if recipe == "denseB":                                                 # patterns 9..15 with covered tiles in between
        return {tiles[(2 * i + 1 + r) % nt]: 15 - i for i in range(min(7, (nt + 1) // 2))}
    if recipe == "full":
        return {t: 15 for t in tiles}
    if recipe == "empty":                                                  # nothing to code: the workgroup leaves early
        return {}
    if recipe == "seven":
        return {t: (15 if i == 0 else three(1)) for i, t in enumerate(spread(2))}
    raise ValueError(recipe)


def layout(w: int, h: int, shift: int = 0, only=None) -> np.ndarray:
    """bool [h/4, w/4]: strip s (64x16 pixels, row-major) takes recipe (s + shift) mod len(RECIPES), so that every recipe meets strips in both
    tile rows of a macro-tile row, the partial last strip column and the partial last strip row.  only: restrict the recipes to these names."""
    names = tuple(only) if only else RECIPES
    want = np.zeros((h // 4, w // 4), dtype=bool)
    xbb, ybb = (w + 63) // 64, (h + 15) // 16
    for s in range(xbb * ybb):
        bx, sy = s % xbb, s // xbb
        ntx, nty = min(8, w // 8 - bx * 8), min(2, h // 8 - sy * 2)
        k = s + shift
        for (ty, tx), pat in _strip_patterns(names[k % len(names)], k // len(names) + sy, ntx, nty).items():
            cy, cx = (sy * 2 + ty) * 2, (bx * 8 + tx) * 2
            for bit in range(4):
                if pat >> bit & 1:
                    want[cy + (bit >> 1), cx + (bit & 1)] = True
    return want


def tile_patterns(cells: np.ndarray) -> np.ndarray:
    """uncovered cells bool [h/4, w/4] -> quadrant pattern per 8x8 tile, int [h/8, w/8]"""
    c = np.asarray(cells, dtype=np.int64)
    return c[0::2, 0::2] | c[0::2, 1::2] << 1 | c[1::2, 0::2] << 2 | c[1::2, 1::2] << 3


def strip_counts(cells: np.ndarray) -> np.ndarray:
    """uncovered cells per 64x16 strip, int [ceil(h/16), ceil(w/64)]"""
    hc, wc = cells.shape
    pad = np.zeros(((hc + 3) // 4 * 4, (wc + 15) // 16 * 16), dtype=np.int64)
    pad[:hc, :wc] = cells
    return pad.reshape(pad.shape[0] // 4, 4, pad.shape[1] // 16, 16).sum(axis=(1, 3))


# ---- value regimes of G and B ------------------------------------------------------------------------------------------------------------------------
# name -> (interior values of a tile with k uncovered cells on the FLAT background, the (color0, minCol, delta) the reference must find).  A coded
# tile holds, per uncovered cell, 7 background pixels (row 0 and column 0 of the cell) and these 9.
def _cyc(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


L = FLAT
REGIMES = {
    "mode0": (lambda k: [0] * (9 * k), (1, L, 0)),                              # 9k zeros outvote 7k background: mode 0 clamps to 1
    "mode255": (lambda k: [255] * (9 * k), (254, L, 0)),                        # mode 255 clamps to 254
    "within1": (lambda k: _cyc([L - 1, L, L + 1], 9 * k), (L, 0, 0)),           # nothing left after color0 +- 1: minCol = delta = 0, every byte 0
    "one_left": (lambda k: [L + 50] * (9 * k), (L + 50, L, 0)),                 # one value left: delta 0, its pixels code as byte 1
    "delta1": (lambda k: _cyc([L + 10, L + 11], 9 * k), (L, L + 10, 1)),        # the pixels equal to minCol: n = -1, byte 0; the others 15
    "delta2": (lambda k: _cyc([L + 10, L + 11, L + 12], 9 * k), (L, L + 10, 2)),
    "delta3": (lambda k: _cyc([L + 10, L + 11, L + 12, L + 13], 9 * k), (L, L + 10, 3)),
    "delta255": (lambda k: _cyc([0, 255], 9 * k), (L, 0, 255)),                 # bytes 1 and 16
    "tie2_up": (lambda k: [L + 100] * (7 * k) + _cyc([150, 160], 2 * k), (L + 100, L, 60)),    # 7k : 7k, the right-most value wins
    "tie2_down": (lambda k: [40] * (7 * k) + _cyc([150, 160], 2 * k), (L, 40, 120)),            # 7k : 7k, the background is the right-most
    "all17": (lambda k: [17 * j for j in range(16)] + [L] * (9 * k - 16), (L, 0, 255)),         # bytes 0 (background) and 1 + j for 17 j: k >= 2
}
TIE3 = "tie3"                                                              # ramp background only, see value_cells
REGIME_NAMES = tuple(REGIMES) + (TIE3,)


def value_cells(want: np.ndarray, bg: str, w: int, h: int, start: int = 0):
    """Regimes for G and B in the uncovered tiles of a shared-coverage layout: ({(plane, cy, cx): 9 values} for plug_image, [(plane, tile y, tile x,
    regime, expected triple)]).  On the flat background the tiles of the sparse strips and those of the dense strips each walk REGIMES in turn (B five
    steps ahead of G).  On the ramp only G carries values and only the three-way tie, in tiles with one uncovered cell: G = 40 + 2 tri(x) gives such a
    cell the background values b x 4 (column 0) and three single ones (row 0); four pixels of 200 and four of 220 tie with b, 220 is the right-most."""
    pats, kinds = tile_patterns(want), strip_counts(want)
    values, expect = {}, []
    seq = {"sparse": start, "dense": start + 3}
    planes_bg = background(w, h, bg)
    for ty, tx in zip(*np.nonzero(pats)):
        pat = int(pats[ty, tx])
        cells = [(2 * ty + (b >> 1), 2 * tx + (b & 1)) for b in range(4) if pat >> b & 1]
        k = len(cells)
        kind = "sparse" if kinds[ty // 2, tx // 8] <= 4 else "dense"
        if bg == "ramp":
            if k != 1:
                continue
            cy, cx = cells[0]
            blk = planes_bg[1, 4 * cy: 4 * cy + 4, 4 * cx: 4 * cx + 4]
            lo = int(min(blk[0].min(), blk[:, 0].min()))
            values[(1, cy, cx)] = [200] * 4 + [220] * 4 + [150]
            expect.append((1, int(ty), int(tx), TIE3, (220, lo, 200 - lo)))
            continue
        for p, ahead in ((1, 0), (2, 5)):
            names = list(REGIMES)
            name = names[(seq[kind] + ahead) % len(names)]
            if name == "all17" and k < 2:
                name = names[(seq[kind] + ahead + 1) % len(names)]
            fill, triple = REGIMES[name]
            v = fill(k)
            for i, (cy, cx) in enumerate(cells):
                values[(p, cy, cx)] = v[9 * i: 9 * i + 9]
            expect.append((p, int(ty), int(tx), name, triple))
        seq[kind] += 1
    return values, expect


# ---- census: what the reference makes of an image --------------------------------------------------------------------------------------------------
def oracle_run(planes: np.ndarray, per_plane: bool = False) -> dict:
    """The reference's side of a case: the seven passes (and the six plane-subset passes), then the three DynamicTileCompressor calls.  Keeps the
    gradient streams for the decoder tests."""
    ora = OracleEncoder(planes)
    grad = [ora.fitting_quad_smooth(sx, sy) for sx, sy in PASSES]
    shared = ~(ora.state("smoothMap")[::4, ::4] != 0)                      # after the seven RGB passes: what no plane has covered
    pp = [ora.fitting_quad_smooth(2, 2, plane_bit=m) for m in PP_MASKS] if per_plane else []
    uncovered = np.stack([~(ora.state("mapSmoothTile", p)[::4, ::4] != 0) for p in range(3)])
    for p in range(3):
        ora.dynamic_tile_compressor(p)
    pix, typ = ora.streams_1d()
    return {"grad": grad, "pp": pp, "shared": shared, "uncovered": uncovered, "pix": pix, "type": typ}


def census(planes: np.ndarray, per_plane: bool = False, run: dict | None = None) -> dict:
    """From the oracle's outputs alone (smoothMap / mapSmoothTile after PP_MASKS, streams_1d): the coded tiles by (pattern, "sparse" | "dense" strip),
    the set of strip valid-cell counts, the (color0, minCol, delta) triples, the stream bytes, the per-plane pattern counts, and one record per coded
    tile: (plane, tile y, tile x, pattern, strip kind, triple, bytes)."""
    run = run or oracle_run(planes, per_plane)
    pix, typ = run["pix"], run["type"]
    tiles, counts, triples, per, records = Counter(), set(), set(), [Counter() for _ in range(3)], []
    tp = pp = 0
    for p in range(3):
        cells = run["uncovered"][p]
        pats, sc = tile_patterns(cells), strip_counts(cells)
        counts |= set(int(v) for v in sc.ravel())
        for ty, tx in zip(*np.nonzero(pats)):
            pat = int(pats[ty, tx])
            n = 16 * bin(pat).count("1")
            kind = "sparse" if sc[ty // 2, tx // 8] <= 4 else "dense"
            triple = tuple(int(v) for v in typ[tp: tp + 3])
            records.append((p, int(ty), int(tx), pat, kind, triple, pix[pp: pp + n]))
            tiles[(pat, kind)] += 1
            per[p][pat] += 1
            triples.add(triple)
            tp += 3; pp += n
    assert (tp, pp) == (typ.size, pix.size), "the streams do not match the coverage"
    return {"tiles": tiles, "strip_counts": counts, "triples": triples, "bytes": set(int(v) for v in np.unique(pix)), "per_plane": per if per_plane else None,
            "records": records}


# ---- the case list ---------------------------------------------------------------------------------------------------------------------------------
def _explicit(w, h, pats):
    want = np.zeros((h // 4, w // 4), dtype=bool)
    for (ty, tx), pat in pats.items():
        for bit in range(4):
            if pat >> bit & 1:
                want[2 * ty + (bit >> 1), 2 * tx + (bit & 1)] = True
    return want


# name -> (w, h, background, want builder): shared coverage
SHARED = {
    "tile8x8_p9": (8, 8, "flat", lambda: _explicit(8, 8, {(0, 0): 9})),
    "tile8x8_p15": (8, 8, "ramp", lambda: _explicit(8, 8, {(0, 0): 15})),
    "row24x8": (24, 8, "flat", lambda: _explicit(24, 8, {(0, 0): 6, (0, 2): 15})),
    "s72x40_flat": (72, 40, "flat", lambda: layout(72, 40, 5)),
    "s72x40_ramp": (72, 40, "ramp", lambda: layout(72, 40, 0)),
    "s264x136_flat": (264, 136, "flat", lambda: layout(264, 136, 0)),
    "s264x136_flat_b": (264, 136, "flat", lambda: layout(264, 136, 7)),
    "s264x136_ramp": (264, 136, "ramp", lambda: layout(264, 136, 3)),
    "s264x264_flat": (264, 264, "flat", lambda: layout(264, 264, 2)),
    "s264x264_sparse": (264, 264, "ramp", lambda: layout(264, 264, 0, only=RECIPES[:10])),
}
# name -> (w, h, background, shifts of the three planes' layouts): coverage per plane, after the plane-subset passes
PER_PLANE = {
    "pp72x40": (72, 40, "ramp", (0, 4, 9)),
    "pp264x136": (264, 136, "flat", (0, 5, 10)),
    "pp264x136_b": (264, 136, "ramp", (3, 8, 13)),
}
NOISE = "noise264x264"
# three layouts of one shape for the batch coder
BATCHES = {"b72x40": ("s72x40_flat", "s72x40_ramp", "tile72x40_alt"), "b264x136": ("s264x136_flat", "s264x136_ramp", "s264x136_flat_b"),
           "b264x264": ("s264x264_flat", NOISE, "s264x264_sparse")}
SHARED["tile72x40_alt"] = (72, 40, "flat", lambda: layout(72, 40, 10))


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """{"planes", "want" ([3, h/4, w/4]), "per_plane", "expect" (value tiles), "run" (oracle_run)}; computed once per process, never changed"""
    if name == NOISE:
        planes = np.random.default_rng(264).integers(0, 256, (3, 264, 264)).astype(np.int32)
        want, per_plane, expect = np.ones((3, 66, 66), dtype=bool), False, []
    elif name in SHARED:
        w, h, bg, build = SHARED[name]
        w2 = build()
        values, expect = value_cells(w2, bg, w, h, start=sum(map(ord, name)))
        planes = plug_image(w, h, w2, values, bg)
        want, per_plane = np.stack([w2] * 3), False
    else:
        w, h, bg, shifts = PER_PLANE[name]
        want, per_plane, expect = np.stack([layout(w, h, s) for s in shifts]), True, []
        planes = plug_image(w, h, want, None, bg)
    for a in (planes, want):
        a.setflags(write=False)
    run = oracle_run(planes, per_plane)
    return {"name": name, "planes": planes, "want": want, "per_plane": per_plane, "expect": expect, "run": run}


SHARED_NAMES = tuple(SHARED) + (NOISE,)
PER_PLANE_NAMES = tuple(PER_PLANE)
ALL_NAMES = SHARED_NAMES + PER_PLANE_NAMES
