"""TEST INFRASTRUCTURE ONLY.  Directed inputs for the GROUPED compact sweep of the fused encode kernel (y2_grad_pass in yaik_amd/csrc/yk_encode2.hip):
a compact pass from 8x8 on evaluates the next pass in the same sweep when `own cells + speculative cells of the next pass <= 16`, the speculative
cells being the next pass's viable tiles under the coverage as it stands BEFORE this pass.  Built with the canvas of tests/gradfit_cases.py (dead
cells, plugs, targets), one 64x16 strip per case, four strips per 256-wide image, a dead strip row underneath.

Which (own, speculative-next) counts exist.  A tile of the first pass is made of whole tiles of the second in the pairs 8x8 -> 8x4 and 4x8 -> 4x4,
and both passes see the same coverage and the same dead cells, so there `next >= own`; 8x8 tiles hold 4 cells, 8x4 and 4x8 tiles 2.  Of the counts
(8, 8), (8, 9), (4, 12), (12, 4), (16, 1), (1, 15) that leaves, per pair (the substitute keeps the sum on the same side of 16, as close as it gets):
  8x8 -> 8x4   (8, 8)  (8, 10) for (8, 9)  (4, 12)  (4, 14) beyond it                      no (12, 4), (16, 1), (1, 15): next >= own, own = 4 n
  8x4 -> 4x8   (8, 8)  (8, 10) for (8, 9)  (4, 12)  (12, 4)  (14, 2) for (16, 1)  (2, 14) for (1, 15)  (2, 16) beyond it    (counts are even)
  4x8 -> 4x4   (8, 8)  (8, 9)  (4, 12)  (2, 14) for (1, 15)  (2, 15) beyond it            no (12, 4), (16, 1): next >= own
A count strip is all plugs: both passes reject every tile.  The scenario strips hold targets; what each claims is asserted from the oracle alone in
tests/test_compact_group_cases.py."""
from __future__ import annotations

import functools

import numpy as np

from tests import gradfit_cases as gc

PAIRS = ((3, 4), (4, 5), (5, 6))                                          # (pass, next pass): 8x8 -> 8x4, 8x4 -> 4x8, 4x8 -> 4x4
GROUP_MAX_CELLS = 16                                                      # yk_encode2.hip, y2_grad_pass: `nCells + nB > 16` (no group)
COUNTS = {0: ((8, 8), (8, 10), (4, 12), (4, 14)),
          1: ((8, 8), (8, 10), (4, 12), (12, 4), (14, 2), (2, 14), (2, 16)),
          2: ((8, 8), (8, 9), (4, 12), (2, 14), (2, 15))}


def _cells(p):
    TX, TY = gc.SHAPES[p]
    return TX // 4, TY // 4


# ---- where the tiles of a strip go: positions (cy, cx) in cells, strip-local --------------------------------------------------------------------
def _spots(k):
    """(origins of first-pass tiles, origins of tiles of the second pass that lie in no first-pass tile), so that no larger tile is free of dead
    cells and the two lists never touch the same cell"""
    if k == 0:      # 8x8 blocks on a checkerboard of blocks; 8x4 tiles: the upper half of the other blocks (lower half dead)
        a = [(2 * by, 2 * bx) for by in range(2) for bx in range(8) if (by + bx) % 2 == 0]
        b = [(2 * by, 2 * bx) for by in range(2) for bx in range(8) if (by + bx) % 2 == 1]
    elif k == 1:    # 8x4 tiles in rows 0 and 2 of the left half (rows 1, 3 dead); 4x8 tiles on even columns of the right half (odd columns dead)
        a = [(cy, cx) for cy in (0, 2) for cx in (0, 2, 4, 6)]
        b = [(cy, cx) for cy in (0, 2) for cx in (8, 10, 12, 14)]
    else:           # 4x8 tiles on even columns of the left half; single cells in rows 0 and 2 of the right half (rows 1, 3 dead)
        a = [(cy, cx) for cy in (0, 2) for cx in (0, 2, 4, 6)]
        b = [(cy, cx) for cy in (0, 2) for cx in range(8, 16)]
    return a, b


def _tiles_for(k, own, spec):
    """numbers of (first-pass tiles, second-pass-only tiles) that give the counts"""
    pa, pb = PAIRS[k]
    ca, cb = _cells(pa)[0] * _cells(pa)[1], _cells(pb)[0] * _cells(pb)[1]
    na = own // ca
    inner = own if k in (0, 2) else 0                                      # cells of the first pass's tiles that are tiles of the second as well
    nb = (spec - inner) // cb
    assert na * ca == own and inner + nb * cb == spec and nb >= 0, (k, own, spec)
    return na, nb


class Strip:
    """one strip's recipe and what it claims: own / spec (cells), fits, the tiles the oracle accepts in the two passes (strip-local cell origins)"""

    def __init__(self, name, k, ops, own, spec, accept_a=(), accept_b=(), rf=3, note="", **more):
        self.name, self.k, self.ops, self.own, self.spec, self.rf, self.note = name, k, ops, own, spec, rf, note
        self.accept_a, self.accept_b = set(accept_a), set(accept_b)
        self.more = more


def _plug_tile(p, cy, cx):
    nx, ny = _cells(p)
    return ("plug", cy, cx, ny, nx)


def _count_strip(k, own, spec, rf=3):
    pa, pb = PAIRS[k]
    na, nb = _tiles_for(k, own, spec)
    sa, sb = _spots(k)
    ops = [_plug_tile(pa, *sa[i]) for i in range(na)] + [_plug_tile(pb, *sb[i]) for i in range(nb)]
    return Strip(f"count{k}_{own}_{spec}", k, ops, own, spec, rf=rf, note="all plugs: both passes reject everything")


def _reject_dec(p, i=0):
    TX, TY = gc.SHAPES[p]
    return (i % 3, TX - 1, TY - 1, -1 if i % 2 == 0 else 1)


def _scenarios(k, rf=3, tag=""):
    """strips with targets; own / spec are what the layout gives (asserted by the CPU test)"""
    pa, pb = PAIRS[k]
    sa, sb = _spots(k)
    inner = 1 if k in (0, 2) else 0
    ca, cb = _cells(pa)[0] * _cells(pa)[1], _cells(pb)[0] * _cells(pb)[1]
    out = []

    def S(name, ops, na, nb, **kw):
        out.append(Strip(f"{name}{k}{tag}", k, ops, na * ca, inner * na * ca + nb * cb, rf=rf, **kw))

    # only the first accepts: a sole survivor in the first pass, plugs in the second (and a second, rejected, first-pass tile)
    nb = 0 if k == 0 else 2                                                # 8x8 -> 8x4: two 8x8 tiles are 8 + 8 cells already
    S("onlyA", [("tgt", pa, sa[0], 1, None), _plug_tile(pa, *sa[2]), _plug_tile(pb, *sb[1]), _plug_tile(pb, *sb[3])][: 2 + nb], 2, nb, accept_a=[sa[0]],
      stage="B1")
    # only the second accepts: plugs in the first pass (lost in stage 1), a sole survivor and a one-pixel reject in the second
    na = 1 if k == 0 else 2
    S("onlyB", [_plug_tile(pa, *sa[0]), _plug_tile(pa, *sa[2])][:na] + [("tgt", pb, sb[1], 0, None), ("tgt", pb, sb[3], 1, _reject_dec(pb, k)), _plug_tile(pb, *sb[5])], na, 3,
      accept_b=[sb[1]], stage="A1")
    # both accept, different variants
    S("both", [("tgt", pa, sa[0], 2, None), ("tgt", pb, sb[2], 5, None), _plug_tile(pa, *sa[3])][:na + 1], na, 1, accept_a=[sa[0]], accept_b=[sb[2]])
    return out


def _special():
    out = []
    # -- the first pass accepts a tile that covers the ORIGIN of a second-pass tile that would otherwise be accepted: planes
    #    8x8 -> 8x4: the 8x8 plane holds two 8x4 tiles, both fitted by the same plane
    out.append(Strip("covers0", 0, [("plane", [(0, 4), (0, 5), (1, 4), (1, 5)], [(0, 6), (1, 6), (2, 4), (2, 6)]), _plug_tile(4, 2, 10)], 4, 6,
                     accept_a=[(0, 4)], covered_b=[(0, 4), (1, 4)]))
    #    8x4 -> 4x8: an L of three live cells: the 8x4 tile (0, x..x+1) and the 4x8 tile (0..1, x) share the origin cell
    out.append(Strip("covers1", 1, [("plane", [(0, 4), (0, 5), (1, 4)], [(0, 6), (1, 6), (2, 4), (2, 5)]), _plug_tile(5, 2, 10)], 2, 4,
                     accept_a=[(0, 4)], covered_b=[(0, 4)]))
    #    4x8 -> 4x4
    out.append(Strip("covers2", 2, [("plane", [(0, 4), (1, 4)], [(0, 5), (1, 5), (2, 4), (2, 5)]), _plug_tile(6, 2, 10)], 2, 3, accept_a=[(0, 4)], covered_b=[(0, 4), (1, 4)]))
    # -- 8x4 then 4x8: the accepted 8x4 tile (1, 4..5) overlaps the 4x8 tile (0..1, 5) without covering its origin (0, 5): both appear
    out.append(Strip("overlap1", 1, [("plane", [(0, 5), (1, 4), (1, 5)], [(0, 6), (1, 6), (2, 4), (2, 5), (2, 6)])], 2, 2,
                     accept_a=[(1, 4)], accept_b=[(0, 5)], overlap=((1, 4), (0, 5))))
    # -- two passes' tiles on ONE origin lane with different survivors: the second pass's target (accepted) is the first cells of a first-pass
    #    tile whose other cells are plugs (rejected); next to it the reverse is not possible (an accepted first-pass tile covers the origin)
    out.append(Strip("shared0", 0, [("tgt", 4, (0, 4), 0, None), ("plug", 1, 4, 1, 2), _plug_tile(3, 2, 10)], 8, 8, accept_b=[(0, 4)], shared=[(0, 4)]))
    out.append(Strip("shared1", 1, [("tgt", 5, (0, 4), 1, None), ("plug", 0, 5, 1, 1), _plug_tile(4, 2, 10)], 4, 2, accept_b=[(0, 4)], shared=[(0, 4)]))
    out.append(Strip("shared2", 2, [("tgt", 6, (0, 4), 0, None), ("plug", 1, 4, 1, 1), _plug_tile(5, 2, 10)], 4, 4, accept_b=[(0, 4)], shared=[(0, 4)]))
    return out


def _apply(cv, col, strip):
    for op in strip.ops:
        if op[0] == "plug":
            _, cy, cx, ncy, ncx = op
            cv.fill(cy, 16 * col + cx, ncy, ncx, "p")
        elif op[0] == "tgt":
            _, p, (cy, cx), variant, dec = op
            nx, ny = _cells(p)
            cv.fill(cy, 16 * col + cx, ny, nx, "p")
            out = cv.place(p, cy, 16 * col + cx, gc._sole(variant, dec, dec is not None)(gc.SHAPES[p], cv.rf), tries=4000, group="Q", strip=strip.name)
            assert out is not None, (strip.name, op)
        else:                                                             # cells of ONE plane 100 + x + y (+ 30 per channel); `corners`: dead cells whose
            _, cells, corners = op                                         # pixel (0, 0), a far corner of the plane's tiles, continues the plane
            dy, dx = np.mgrid[0:4, 0:4]
            for n, (cy, cx) in enumerate(list(cells) + list(corners)):
                level = 100 + 4 * cx + 4 * cy + 30 * np.arange(3)
                cv.lat[(cy, 16 * col + cx)] = level
                if n < len(cells):
                    cv.kind[cy, 16 * col + cx] = "t"
                    cv.tiles.append((4 * cy, 4 * (16 * col + cx), level[:, None, None] + dx[None] + dy[None]))


def _image(name, strips, rf, seed, w=256):
    cv = gc.Canvas(w, 32, rf, seed)
    for col, s in enumerate(strips):
        _apply(cv, col, s)
    return cv


def _edge_image(w, seed):
    """the last strip column of an image 8 mod 16 wide: two cell columns inside the image.  8x4 -> 4x8 (the only pair whose first pass fits two
    columns): an 8x4 tile of plugs in row 0 with a live cell under its first cell (a 4x8 tile on the same origin lane), and in row 2 a plane
    against the edge whose far corners are clamped reads (place_ramp: the cells under it become plugs, an 8x4 tile and two 4x8 tiles more)"""
    cv = gc.Canvas(w, 32, 3, seed)
    cx0 = w // 4 - 2
    cv.fill(0, cx0, 1, 2, "p")
    cv.fill(1, cx0, 1, 1, "p")
    cv.place_ramp(4, 2, cx0, (1, 0), np.array((210, 220, 230), np.int64), group="Q", strip="edge")
    strip = Strip(f"edge{w}", 1, [], 6, 6, accept_a=[(2, cx0 % 16)], edge=True)
    return cv, strip


@functools.lru_cache(maxsize=None)
def _build():
    """{image name: (Canvas, [(strip column, Strip)])}"""
    images = {}
    for k in range(3):
        strips = [_count_strip(k, own, spec) for own, spec in COUNTS[k]] + _scenarios(k)
        for i in range(0, len(strips), 4):
            part = strips[i: i + 4]
            images[f"q{k}_{i // 4}"] = (_image(f"q{k}_{i // 4}", part, 3, 8000 + 10 * k + i), list(enumerate(part)))
    sp = _special()
    for i in range(0, len(sp), 4):
        part = sp[i: i + 4]
        images[f"qs_{i // 4}"] = (_image(f"qs_{i // 4}", part, 3, 8100 + i), list(enumerate(part)))
    for rf in (0, 64):                                                    # one image per reject factor: the scenarios of the three pairs that fit its width
        part = [_scenarios(k, rf, f"_rf{rf}")[1 if rf == 0 else 0] for k in range(3)] + [_count_strip(1, 8, 8, rf)]
        images[f"q_rf{rf}"] = (_image(f"q_rf{rf}", part, rf, 8200 + rf), list(enumerate(part)))
    for w in (72, 136):
        cv, strip = _edge_image(w, 8300 + w)
        images[f"q_edge{w}"] = (cv, [(w // 64, strip)])
    return images


NAMES = tuple(_build())


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """{"name", "planes", "rf", "strips": [(column, Strip)], "census"}; "<name>@rot1" / "@rot2": the channels rotated (frames for a batch)"""
    base, _, rot = name.partition("@rot")
    cv, strips = _build()[base]
    planes = cv.render() if not rot else np.ascontiguousarray(np.roll(case(base)["planes"], int(rot), axis=0))
    planes.setflags(write=False)
    return {"name": name, "planes": planes, "rf": cv.rf, "strips": () if rot else tuple(strips), "census": gc.census(planes, cv.rf)}


# ---- what a strip holds, from the census ----------------------------------------------------------------------------------------------------------
def spec_cells(c: dict, p: int, col: int, before: int) -> int:
    """cells of pass p's viable tiles in strip (0, col) under the coverage as it stands before pass `before`: no dead cell, inside the image,
    origin cell not covered by a tile the oracle accepted in a pass < before"""
    cs = c["census"]
    _, h, w = c["planes"].shape
    nx, ny = _cells(p)
    cov = covered_before(c, before)
    n = 0
    for cy in range(0, 4, ny):
        for cx in range(16 * col, 16 * col + 16, nx):
            if 4 * (cx + nx) > w or 4 * (cy + ny) > h:
                continue
            if cs["dead"][cy: cy + ny, cx: cx + nx].any() or cov[cy, cx]:
                continue
            n += nx * ny
    return n


def covered_before(c: dict, before: int) -> np.ndarray:
    cs = c["census"]
    _, h, w = c["planes"].shape
    cov = np.zeros((h // 4, (w + 63) // 64 * 16), bool)
    for (p, ty, tx), rec in cs["tiles"].items():
        if p < before and rec["accepted"]:
            nx, ny = _cells(p)
            cov[ty * ny: ty * ny + ny, tx * nx: tx * nx + nx] = True
    return cov


def accepted(c: dict, p: int, col: int) -> set:
    """strip-local cell origins of the tiles of pass p that the oracle's bitmap holds in strip (0, col)"""
    _, h, w = c["planes"].shape
    nx, ny = _cells(p)
    t = gc.bitmap_tiles(c["census"]["grad"][p][1], p, w, h)
    return {(ty * ny, tx * nx - 16 * col) for ty, tx in zip(*np.nonzero(t)) if ty * ny < 4 and 16 * col <= tx * nx < 16 * col + 16}


def stage1_lost(c: dict, p: int, cy: int, cx: int) -> bool:
    """the compact path's first stage (streams 0 and 3: channel 0 of the raw / Round6 corners, channels 0 and 1 of the Round6P corners) already
    fails all six variants of the tile whose origin is cell (cy, cx) (image cells)"""
    TX, TY = gc.SHAPES[p]
    planes = c["planes"]
    cur = planes[:, 4 * cy: 4 * cy + TY, 4 * cx: 4 * cx + TX].astype(np.int64)
    corners = gc.tile_corners(planes, 4 * cx, 4 * cy, TX, TY)
    fail = np.abs(cur[None] - gc._blends(corners[None], TX, TY)[0]) > c["rf"]          # [6, 3, TY, TX]
    return bool(all(fail[v, 0].any() for v in range(4)) and all(fail[v, :2].any() for v in (4, 5)))


BATCHES = tuple(tuple([n, f"{n}@rot1", f"{n}@rot2"]) for n in NAMES)
