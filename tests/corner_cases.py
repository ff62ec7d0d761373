"""TEST INFRASTRUCTURE ONLY.  Directed inputs for the encoder's corner colour streams (`rgbStream`, yk_corners.hip): images that set the tile
bitmaps of all seven gradient passes on purpose, a sequential model of the emission and a census of what every case really holds.

Images.  R = 30 + zig(x), G = 30 + zig(y), B = 20 + floor(100 (x / w + y / h)).  zig() is a zigzag whose slope flips every P pixels (its pitch)
between +3 and -2 (or +2 and -3, see zig), band by band: `xb` / `yb` list (length, pitch) bands along x / y, every band a multiple of twice its
pitch (but the last), so every band starts at 0 going up and the kinks lie at multiples of P.  A tile wider than the x pitch or taller than the y
pitch spans a kink and fails by 2 P >= 8; a
tile inside one segment of both is linear in every channel and fits exactly; so a (Px, Py) region gives its tiles to the first pass whose shape
fits.  B is a slow drift over the whole image (within one level of linear inside any tile) that tells far-apart places with equal R and G apart;
neighbouring lattice points differ by 12 in R or G, three steps of Round6, so a colour taken from the wrong lattice point or written at the wrong
offset changes bytes (fewer than one pair in fifty of consecutive colours of a stream are equal, tests/test_corner_cases.py).  The slopes are at
most 3 per channel, which is what the clamped corner reads of the last tile column and row bend a fit by: under the reject factor.
Plug cells are those of tests/range1d_cases.py: +60 on the interior 3 x 3 of a 4 x 4 cell of R fails every tile over that cell and leaves the
pixels that other tiles read as corners alone.  A plugged tile of pass p decays into the tiles of the later passes that still fit beside the plug.

model_streams() restates the reference's emission (encoder/EncoderContext.cpp:3783-3785, 4001-4021, 4113-4132) from the rule alone, with the
BITMAPS as input: passes in file order, tiles in swizzled bit order, corners TL, TR, BL, BR; a lattice point that is mapped already is skipped,
otherwise it is mapped and CompressF(Round6(pixel), 250) of R, G, B is appended, the pixel read at (min(4 ly, h - 1), min(4 lx, w - 1)).
defect= switches in one deliberate error; tests/test_corner_cases.py names the case that sees each.

census() reads back, from the oracle's bitmaps and stream lengths alone, what a case holds, per pass and per 1024 bitmap bytes (one workgroup of
yk_corner_stream_body): colours owned, run offset, byte values, the same-byte relations of yk_corner_owner_body, corners lost to earlier passes and
to other bytes / swizzle blocks / workgroups of the same pass, colours from clamped reads, and the neighbour placements of every pair of passes.

Groups: a every byte value, b cross-pass and cross-boundary ownership, c runs and the LDS cap, d edges and odd sizes, e batches of three.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle.pyoracle import PASSES, OracleEncoder
from tests.graddec_cases import bit_tile, geo, set_tiles, tile_bit

PLUG = 60
NONE = 0xFFFFFFFF
DEFECTS = ("corner_order", "later_pass_wins", "larger_bit_wins", "row_major", "no_clamp", "no_plus127", "no_round6", "left_across_wrap", "upright_owns_tl")
RELATIONS = ("left", "up", "upLeft", "upRight")
KCAP = 8192                                                                     # colours a workgroup collects in LDS (yk_corner_stream_body)


# ---- images ------------------------------------------------------------------------------------------------------------------------------------
def zig(n: int, bands) -> np.ndarray:
    """zigzag over n pixels; bands = [(length, pitch)], the last band is cut at n.  Inside a band the slope flips every `pitch` pixels: +3 / -2 while
    the band climbs, +2 / -3 while it comes down again (M pixels each, M the largest power of two up to 128 that holds whole periods and halves a
    whole number of times into the band), so lattice points one period apart differ too; a band that has no such M is a plain +3 / -3 zigzag.  Every
    band returns to 0 at its end."""
    out, x0 = np.zeros(n, dtype=np.int64), 0
    for i, (length, pitch) in enumerate(bands):
        x1 = n if i == len(bands) - 1 else x0 + length
        assert x1 == n or (length % (2 * pitch) == 0 and x0 % 64 == 0), (bands, i)
        half = next((m for m in (128, 64, 32, 16, 8) if length % (2 * m) == 0 and m % (2 * pitch) == 0), 0)
        t = np.arange(x1 - x0)
        up = (t % (2 * pitch)) < pitch
        if half:
            climb = (t % (2 * half)) < half
            slope = np.where(climb, np.where(up, 3, -2), np.where(up, 2, -3))
        else:
            slope = np.where(up, 3, -3)
        out[x0:x1] = np.concatenate([[0], np.cumsum(slope)[:-1]])
        x0 = x1
    assert x0 == n and out.min() >= 0
    return out


def image(w: int, h: int, xb, yb, plugs=None) -> np.ndarray:
    """int32 planes [3, h, w]; xb / yb: pitch bands along x / y (an int = one band); plugs: bool [h/4, w/4]"""
    xb = [(w, xb)] if isinstance(xb, int) else list(xb)
    yb = [(h, yb)] if isinstance(yb, int) else list(yb)
    fx, gy = zig(w, xb)[None, :], zig(h, yb)[:, None]
    drift = 20 + (100 * (np.arange(w, dtype=np.int64)[None, :] * h + np.arange(h, dtype=np.int64)[:, None] * w)) // (w * h)
    planes = np.stack([30 + fx + 0 * gy, 30 + gy + 0 * fx, drift]).astype(np.int32)
    if plugs is not None:
        plugs = np.asarray(plugs, dtype=bool)
        assert plugs.shape == (h // 4, w // 4), (plugs.shape, w, h)
        for cy, cx in zip(*np.nonzero(plugs)):
            planes[0, 4 * cy + 1: 4 * cy + 4, 4 * cx + 1: 4 * cx + 4] += PLUG
    assert planes.min() >= 0 and planes.max() <= 255                            # no clip, no wrap
    return planes


def scatter(w: int, h: int, one_in: int, seed: int) -> np.ndarray:
    """bool [h/4, w/4]: about one cell in `one_in`, by a fixed hash of the cell's coordinates"""
    cy, cx = np.mgrid[0:h // 4, 0:w // 4].astype(np.uint64)
    v = (cx * np.uint64(73856093)) ^ (cy * np.uint64(19349663)) ^ np.uint64(83492791 * (seed + 1))
    v = (v * np.uint64(2654435761)) >> np.uint64(11)
    return (v % np.uint64(one_in)) == 0


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def _colour(planes, w, h, ly, lx, defect):
    y, x = min(4 * ly, h - 1), min(4 * lx, w - 1)
    if defect == "no_clamp":
        y, x = (h - 4 if 4 * ly == h else 4 * ly), (w - 4 if 4 * lx == w else 4 * lx)
    v = planes[:3, y, x].astype(np.int64)
    r6 = v if defect == "no_round6" else ((v >> 2) << 2) | (v >> 6)
    return ((r6 * 250 + (0 if defect == "no_plus127" else 127)) // 255).tolist()


def _points(sx, sy, tx, ty):
    lx, ly, dx, dy = (tx << sx) >> 2, (ty << sy) >> 2, 1 << (sx - 2), 1 << (sy - 2)
    return ((ly, lx), (ly, lx + dx), (ly + dy, lx), (ly + dy, lx + dx))


def same_byte_relations(sx: int, sy: int, w: int, byte: int, bit: int) -> dict:
    """the neighbours of tile `bit` inside its own bitmap byte, as yk_corner_owner_body defines them, and the three places where the byte wraps:
    "wrapLeft" (bit k - 1 set, the tile in column 0), "wrapUpLeft" (bit k - 5, column 0), "wrapUpRight" (bit k - 3, column 3)"""
    tpr = geo(sx, sy, w, 8)["tpr"]
    k, col, two = bit & 7, (bit % geo(sx, sy, w, 8)["bit_count"]) % tpr, tpr == 4
    has = lambda j: j >= 0 and bool((byte >> j) & 1)
    return {"left": k >= 1 and col != 0 and has(k - 1), "up": two and has(k - 4), "upLeft": two and col != 0 and has(k - 5),
            "upRight": two and k >= 4 and col != 3 and has(k - 3),
            "wrapLeft": k >= 1 and col == 0 and has(k - 1), "wrapUpLeft": two and col == 0 and has(k - 5), "wrapUpRight": two and k >= 4 and col == 3 and has(k - 3),
            "k": k, "col": col}


def model_streams(bitmaps, planes, w: int, h: int, defect: str | None = None) -> dict:
    """"streams": the seven colour streams (uint8); "owner": uint32 [h/4 + 1, w/4 + 1], pass << 27 | bit << 2 | corner of the tile corner that emitted
    the point, 0xFFFFFFFF = untouched; "ordinal": int64, the colour's place within its pass's stream, -1 = none"""
    assert defect is None or defect in DEFECTS, defect
    lat_h, lat_w = h // 4 + 1, w // 4 + 1
    owner = np.full((lat_h, lat_w), NONE, dtype=np.uint32)
    ordinal = np.full((lat_h, lat_w), -1, dtype=np.int64)
    mapped = np.zeros((lat_h, lat_w), dtype=bool)
    tiles = [set_tiles(sx, sy, w, bitmaps[p]) for p, (sx, sy) in enumerate(PASSES)]
    last_pass = np.full((lat_h, lat_w), -1, dtype=np.int64)
    last_bit = [dict() for _ in range(7)]
    if defect in ("later_pass_wins", "larger_bit_wins"):
        for p, (sx, sy) in enumerate(PASSES):
            for bit, tx, ty in tiles[p]:
                for pt in _points(sx, sy, tx, ty):
                    last_pass[pt] = p
                    last_bit[p][pt] = bit
    streams = []
    for p, (sx, sy) in enumerate(PASSES):
        out = []
        order = sorted(tiles[p], key=lambda t: (t[2], t[1])) if defect == "row_major" else tiles[p]
        bm = np.asarray(bitmaps[p], dtype=np.uint8)
        for bit, tx, ty in order:
            pts = _points(sx, sy, tx, ty)
            skip = set()
            if defect in ("left_across_wrap", "upright_owns_tl"):
                rel = same_byte_relations(sx, sy, w, int(bm[bit >> 3]), bit)
                if defect == "left_across_wrap" and rel["wrapLeft"]:
                    skip = {0, 2}                                               # "the left neighbour owns TL and BL": no atomic for them
                if defect == "upright_owns_tl" and rel["upRight"]:
                    skip = {0}
            for q in ((0, 2, 1, 3) if defect == "corner_order" else (0, 1, 2, 3)):
                pt = pts[q]
                if mapped[pt] or q in skip:
                    continue
                if defect == "later_pass_wins" and last_pass[pt] > p:
                    continue
                if defect == "larger_bit_wins" and last_bit[p][pt] != bit:
                    continue
                mapped[pt] = True
                owner[pt] = (p << 27) | (bit << 2) | q
                ordinal[pt] = len(out) // 3
                out += _colour(planes, w, h, pt[0], pt[1], defect)
        streams.append(np.asarray(out, dtype=np.uint8))
    return {"streams": streams, "owner": owner, "ordinal": ordinal}


# ---- census --------------------------------------------------------------------------------------------------------------------------------------
def oracle_run(planes: np.ndarray, rf: int = 3) -> list:
    """[(count, bitmap, rgbStream)] of the seven passes"""
    ora = OracleEncoder(planes)
    return [ora.fitting_quad_smooth(sx, sy, rf) for sx, sy in PASSES]


PLACEMENTS = ("left", "right", "above", "below", "diagonal")


def census_of(run: list, w: int, h: int) -> dict:
    """From the oracle's bitmaps (and its stream lengths, as a check).  "groups"[p] = one record per 1024 bitmap bytes of pass p: {"tot", "offset"
    (bytes into the pass's stream), "bytes" (values), "relations" {(name, k, col)}, "combos" {the relations one tile has together}, "lost_earlier", "lost_byte", "lost_block", "lost_group", "clamped"};
    "byte_values"[p]; "pairs" {(p, q, placement of the q tile seen from the p tile, q first in bit order)} for p <= q (p == q: within the pass, the
    third entry then "byte" | "block" | "group" | "far": what lies between the two tiles); "corner_points": owner keys of the image's four corners."""
    bitmaps = [bm for _, bm, _ in run]
    lat_h, lat_w = h // 4 + 1, w // 4 + 1
    owner = np.full((lat_h, lat_w), NONE, dtype=np.uint64)
    tiles = [set_tiles(sx, sy, w, bitmaps[p]) for p, (sx, sy) in enumerate(PASSES)]
    for p, (sx, sy) in enumerate(PASSES):
        for bit, tx, ty in tiles[p]:
            assert ((tx + 1) << sx) <= w and ((ty + 1) << sy) <= h, "a bit outside the image is set"
            for q, pt in enumerate(_points(sx, sy, tx, ty)):
                owner[pt] = min(int(owner[pt]), (p << 27) | (bit << 2) | q)
    groups, byte_values, pairs = [], [], set()
    cell = np.full((h // 4, w // 4, 2), -1, dtype=np.int64)                      # which (pass, bit) covers a 4x4 cell
    for p, (sx, sy) in enumerate(PASSES):
        for bit, tx, ty in tiles[p]:
            cell[(ty << sy) >> 2:((ty + 1) << sy) >> 2, (tx << sx) >> 2:((tx + 1) << sx) >> 2] = (p, bit)
    for p, (sx, sy) in enumerate(PASSES):
        g = geo(sx, sy, w, h)
        bm = np.asarray(bitmaps[p], dtype=np.uint8)
        assert bm.size == g["nbytes"]
        recs = [{"tot": 0, "offset": 0, "bytes": set(), "relations": set(), "combos": set(), "lost_earlier": 0, "lost_byte": 0, "lost_block": 0, "lost_group": 0, "clamped": 0}
                for _ in range(-(-bm.size // 1024))]
        for k in range(len(recs)):
            recs[k]["bytes"] = set(int(v) for v in np.unique(bm[1024 * k: 1024 * k + 1024]))
        for bit, tx, ty in tiles[p]:
            r = recs[bit >> 13]
            rel = same_byte_relations(sx, sy, w, int(bm[bit >> 3]), bit)
            r["relations"] |= {(n, rel["k"], rel["col"]) for n in rel if n not in ("k", "col") and rel[n]}
            r["combos"].add(tuple(n for n in RELATIONS if rel[n]))
            for q, pt in enumerate(_points(sx, sy, tx, ty)):
                key = int(owner[pt])
                if key == ((p << 27) | (bit << 2) | q):
                    r["tot"] += 1
                    r["clamped"] += int(4 * pt[0] == h or 4 * pt[1] == w)
                    continue
                op, ob = key >> 27, (key >> 2) & ((1 << 25) - 1)
                if op < p:
                    r["lost_earlier"] += 1
                elif ob >> 3 == bit >> 3:
                    r["lost_byte"] += 1
                elif ob // g["bit_count"] == bit // g["bit_count"]:
                    r["lost_block"] += 1
                elif ob >> 13 == bit >> 13:
                    r["lost_group"] += 1
                else:
                    r["lost_far"] = r.get("lost_far", 0) + 1
            # neighbour placements: the cells around this tile
            x0, y0, x1, y1 = (tx << sx) >> 2, (ty << sy) >> 2, ((tx + 1) << sx) >> 2, ((ty + 1) << sy) >> 2
            around = [("left", x0 - 1, y) for y in range(y0, y1)] + [("right", x1, y) for y in range(y0, y1)] + [("above", x, y0 - 1) for x in range(x0, x1)] + \
                     [("below", x, y1) for x in range(x0, x1)] + [("diagonal", x, y) for x in (x0 - 1, x1) for y in (y0 - 1, y1)]
            for where, cx, cy in around:
                if 0 <= cx < w // 4 and 0 <= cy < h // 4 and cell[cy, cx, 0] >= 0:
                    q, qbit = int(cell[cy, cx, 0]), int(cell[cy, cx, 1])
                    if q > p:
                        pairs.add((p, q, where, qbit < bit))
                    elif q == p and qbit != bit:
                        sep = "byte" if qbit >> 3 != bit >> 3 else None
                        if qbit // g["bit_count"] != bit // g["bit_count"]:
                            sep = "block"
                        if qbit >> 13 != bit >> 13:
                            sep = "group"
                        if sep:
                            pairs.add((p, p, where, sep))
        off = 0
        for r in recs:
            r["offset"] = 3 * off
            off += r["tot"]
        assert 3 * off == run[p][2].size, ("pass", p, "owns", off, "colours, the oracle's stream holds", run[p][2].size, "bytes")
        assert len(tiles[p]) == run[p][0]
        groups.append(recs)
        byte_values.append(set().union(*[r["bytes"] for r in recs]) if recs else set())
    corner_points = [int(owner[y, x]) for y, x in ((0, 0), (0, lat_w - 1), (lat_h - 1, 0), (lat_h - 1, lat_w - 1))]
    return {"groups": groups, "byte_values": byte_values, "pairs": pairs, "counts": [c for c, _, _ in run], "corner_points": corner_points,
            "owner": owner.astype(np.uint32)}


# ---- builders --------------------------------------------------------------------------------------------------------------------------------------
BANDS_A = [(64, 32), (64, 16), (64, 8), (64, 4)]
BANDS_B = [(64, 4), (64, 32), (64, 8), (64, 16)]
BANDS_C = [(64, 8), (64, 4), (64, 16), (64, 32)]


def _bands(n: int, bands):
    """the bands cut to n pixels"""
    out, x = [], 0
    for length, pitch in bands:
        if x >= n:
            break
        out.append((min(length, n - x), pitch)); x += length
    return out


def _mosaic(w, h, xb, yb, one_in, seed):
    return image(w, h, _bands(w, xb), _bands(h, yb), scatter(w, h, one_in, seed) if one_in else None)


def _bytes_image(p: int, w: int, h: int, values) -> np.ndarray:
    """byte i of pass p's bitmap = values[i]: the pitch of p's shape everywhere, one plugged cell in every tile whose bit is clear"""
    sx, sy = PASSES[p]
    n = geo(sx, sy, w, h)["nbytes"]
    assert len(values) == n, (p, w, h, n, len(values))
    plugs = np.zeros((h // 4, w // 4), dtype=bool)
    cw, ch = 1 << (sx - 2), 1 << (sy - 2)
    for bit in range(8 * n):
        if not (values[bit >> 3] >> (bit & 7)) & 1:
            tx, ty = bit_tile(sx, sy, w, bit)
            c = (5 * bit + 3) % (cw * ch)
            plugs[ty * ch + c // cw, tx * cw + c % cw] = True
    return image(w, h, 1 << sx, 1 << sy, plugs)


PERM = [(167 * k + 5) % 256 for k in range(256)]
BYTES_CASES = {}                                                               # name -> (pass, w, h, values)
for _i in range(4):
    BYTES_CASES[f"bytes_p0_{_i}"] = (0, 512, 256, PERM[64 * _i: 64 * _i + 64])
    BYTES_CASES[f"bytes_p1_{_i}"] = (1, 256, 256, PERM[64 * _i: 64 * _i + 64])
BYTES_CASES.update({"bytes_p2": (2, 512, 512, PERM), "bytes_p3": (3, 512, 256, PERM), "bytes_p4": (4, 512, 128, PERM), "bytes_p5": (5, 256, 256, PERM),
                    "bytes_p6": (6, 256, 128, PERM)})


def _keep_only(w, h, cells) -> np.ndarray:
    """plugs everywhere but in the listed cells (cx, cy)"""
    plugs = np.ones((h // 4, w // 4), dtype=bool)
    for cx, cy in cells:
        plugs[cy, cx] = False
    return plugs


def _quarter(w, h):
    plugs = np.ones((h // 4, w // 4), dtype=bool)
    plugs[0::2, 0::2] = False
    return plugs


def _checker(w, h):
    cy, cx = np.mgrid[0:h // 4, 0:w // 4]
    return (cx + cy) % 2 == 1


# runs: 1024 pixels wide, so 1024 bytes of the 4x4 pass are 128 rows.  Columns below 64 have x pitch 8, the others 4; in every 128-row group the
# rows below 64 have y pitch 8, the others 4.  Around T = the 4x4 tile at (64, 64) of a group: H = the 8x4 tile left of it (owns T's TL and BL),
# V = the 4x8 tile above it (TL and TR), D = the 8x4 tile above-left (TL only).  All other cells are plugged, so a group owns 1 (H and V), 2 (H),
# 3 (D) or 4 (none) colours, and 0 when T is plugged too.
# The two sequences walk every (colours before the run mod 4, run length 1..4) once, with an empty group between two others.
RUN_TOTS = {"runs_a": (1, 1, 1, 4, 0, 1, 2, 3, 4, 2), "runs_b": (3, 3, 4, 2, 0, 4, 1, 3, 3, 2)}


def _runs(tots) -> np.ndarray:
    w, h = 1024, 128 * len(tots)
    keep = []
    for k, t in enumerate(tots):
        cy = 32 * k + 16
        if t == 0:
            continue
        keep.append((16, cy))
        if t in (1, 2):
            keep += [(14, cy), (15, cy)]
        if t == 1:
            keep += [(16, cy - 2), (16, cy - 1)]
        if t == 3:
            keep += [(14, cy - 1), (15, cy - 1)]
    yb = [(64, 8), (64, 4)] * len(tots)
    return image(w, h, [(64, 8), (960, 4)], yb, _keep_only(w, h, keep))


def q_first_witnesses(p: int, q: int, w: int, h: int):
    """every ((tx, ty) of a pass p tile, (qx, qy) of a pass q tile) of a w x h image where the two touch (side or corner, no overlap) and the q tile
    has the smaller bit index, by enumeration.  For most pairs there are few: the later pass has the smaller tiles, so its indices grow faster."""
    (psx, psy), (qsx, qsy) = PASSES[p], PASSES[q]
    for ty in range(h >> psy):
        for tx in range(w >> psx):
            x0, y0, x1, y1 = tx << psx, ty << psy, (tx + 1) << psx, (ty + 1) << psy
            pbit = tile_bit(psx, psy, w, tx, ty)
            seen = set()
            for cx in range(x0 - 4, x1 + 4, 4):
                for cy in range(y0 - 4, y1 + 4, 4):
                    if not (0 <= cx < w and 0 <= cy < h) or (x0 <= cx < x1 and y0 <= cy < y1):
                        continue
                    qx, qy = cx >> qsx, cy >> qsy
                    if ((qx << qsx) < x1 and ((qx + 1) << qsx) > x0 and (qy << qsy) < y1 and ((qy + 1) << qsy) > y0) or (qx, qy) in seen:
                        continue                                               # the q tile over that cell would overlap the p tile
                    seen.add((qx, qy))
                    if ((qx + 1) << qsx) <= w and ((qy + 1) << qsy) <= h and tile_bit(qsx, qsy, w, qx, qy) < pbit:
                        yield (tx, ty), (qx, qy)


@functools.lru_cache(maxsize=None)
def _origin_plugs(w: int = 256, h: int = 256) -> tuple:
    """plug maps of 256 x 256 images that hold, between them, one witness of q_first_witnesses for every pair p < q that has any: all cells are
    plugged but those of the chosen tiles.  The pairs with the fewest witnesses choose first; the two tiles of a witness keep a cell's distance from
    every tile chosen before (so that no two of them make up a larger tile), but a pass p tile that is there already may serve again; a pair that
    finds no room goes to the next image.  A witness that the oracle does not bear out (the reference asks only whether a tile's first cell is
    free, so a 4x8 tile may form over a free 4x4 cell and half of an 8x4 tile below it) is struck and the images are made again."""
    banned = set()
    while True:
        out, chosen = _origin_try(w, h, banned)
        bad = set()
        for k, plugs in enumerate(out):
            pairs = census_of(oracle_run(image(w, h, 32, 32, plugs)), w, h)["pairs"]
            bad |= {(p, q, wit) for kk, p, q, wit in chosen if kk == k and not any((a, b, f) == (p, q, True) for a, b, _, f in pairs)}
        if not bad:
            return tuple(out)
        banned |= bad


def _origin_try(w, h, banned):
    todo = [(len(ws), p, q, ws) for p in range(7) for q in range(p + 1, 7) for ws in [[x for x in q_first_witnesses(p, q, w, h) if (p, q, x) not in banned]] if ws]
    todo.sort(key=lambda t: t[:3])
    out, chosen = [], []

    def cells(pas, t):
        sx, sy = PASSES[pas]
        return (t[1] << sy) >> 2, ((t[1] + 1) << sy) >> 2, (t[0] << sx) >> 2, ((t[0] + 1) << sx) >> 2

    while todo:
        used, plugs, there, later = np.zeros((h // 4 + 2, w // 4 + 2), dtype=bool), np.ones((h // 4, w // 4), dtype=bool), set(), []
        for n, p, q, ws in todo:
            for pt, qt in ws:
                new = [(pas, t) for pas, t in ((p, pt), (q, qt)) if (pas, t) not in there]
                if (q, qt) in there or any(used[y0:y1 + 2, x0:x1 + 2].any() for y0, y1, x0, x1 in (cells(*t) for t in new)):     # the tile and the ring around it
                    continue
                for t in new:
                    y0, y1, x0, x1 = cells(*t)
                    used[y0 + 1:y1 + 1, x0 + 1:x1 + 1] = True
                    plugs[y0:y1, x0:x1] = False
                    there.add(t)
                chosen.append((len(out), p, q, (pt, qt)))
                break
            else:
                later.append((n, p, q, ws))
        assert len(later) < len(todo)
        todo = later
        out.append(plugs)
    return out, chosen


ORIGIN_NAMES = ("origin_256_a", "origin_256_b")


def _origin(k: int) -> np.ndarray:
    return image(256, 256, 32, 32, _origin_plugs()[k])


_BUILDERS = {n: functools.partial(_bytes_image, *a) for n, a in BYTES_CASES.items()}
_GROUP = {n: "a" for n in BYTES_CASES}


def _add(name, group, fn):
    _BUILDERS[name] = fn
    _GROUP[name] = group


_add("mosaic_256_a", "b", lambda: _mosaic(256, 256, BANDS_A, BANDS_A, 9, 1))
_add("mosaic_256_b", "b", lambda: _mosaic(256, 256, BANDS_B, BANDS_C, 7, 2))
_add("mosaic_256_c", "b", lambda: _mosaic(256, 256, BANDS_C, BANDS_B, 5, 3))
for _k, _n in enumerate(ORIGIN_NAMES):
    _add(_n, "b", functools.partial(_origin, _k))
_add("full_p6_512x512", "b", lambda: image(512, 512, 4, 4))
_add("full_p4_512x1024", "b", lambda: image(512, 1024, 8, 4))
_add("quarter_512x256", "c", lambda: image(512, 256, 4, 4, _quarter(512, 256)))
_add("checker_512x256", "c", lambda: image(512, 256, 4, 4, _checker(512, 256)))
_add("checker_512x512", "c", lambda: image(512, 512, 4, 4, _checker(512, 512)))
for _n, _t in RUN_TOTS.items():
    _add(_n, "c", functools.partial(_runs, _t))
_add("mosaic_200x136", "d", lambda: _mosaic(200, 136, BANDS_B, BANDS_A, 11, 4))
_add("mosaic_72x40", "d", lambda: _mosaic(72, 40, [(64, 16), (64, 4)], [(64, 8)], 0, 0))
_add("small_72x40", "d", lambda: image(72, 40, 4, 4, scatter(72, 40, 3, 5)))
_add("clean_200x136", "d", lambda: _mosaic(200, 136, BANDS_A, BANDS_C, 0, 0))
_add("plugged_72x40", "d", lambda: image(72, 40, 4, 4, np.ones((10, 18), dtype=bool)))
_add("p0_64x64", "d", lambda: image(64, 64, 32, 32))
_add("p0_192x64", "d", lambda: image(192, 64, 16, 16, scatter(192, 64, 40, 8)))
_add("plugged_512x256", "e", lambda: image(512, 256, 4, 4, np.ones((64, 128), dtype=bool)))
_add("sparse_512x256", "e", lambda: image(512, 256, 4, 4, ~scatter(512, 256, 13, 6)))
_add("plugged_200x136", "e", lambda: image(200, 136, 4, 4, np.ones((34, 50), dtype=bool)))
_add("busy_200x136", "e", lambda: _mosaic(200, 136, BANDS_C, BANDS_B, 2, 7))

ALL_NAMES = tuple(_BUILDERS)
BYTES_NAMES = tuple(BYTES_CASES)
WHOLE_IMAGE_EDGE_NAMES = tuple(n for n in ALL_NAMES if _GROUP[n] in ("b", "d"))
# dense, empty, sparse: a frame-stride error swaps data that differ
BATCHES = {"b512x256": ("checker_512x256", "plugged_512x256", "sparse_512x256"), "b200x136": ("busy_200x136", "plugged_200x136", "mosaic_200x136"),
           "b72x40": ("small_72x40", "plugged_72x40", "mosaic_72x40")}
STALE = ("checker_512x256", "sparse_512x256", "plugged_512x256")


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """{"name", "group", "planes", "w", "h", "run" (the oracle's seven passes)}; computed once per process, never changed"""
    planes = _BUILDERS[name]()
    planes.setflags(write=False)
    h, w = planes.shape[1:]
    run = oracle_run(planes)
    for _, bm, rgb in run:
        bm.setflags(write=False); rgb.setflags(write=False)
    return {"name": name, "group": _GROUP[name], "planes": planes, "w": w, "h": h, "run": run}


@functools.lru_cache(maxsize=None)
def model(name: str) -> dict:
    c = case(name)
    m = model_streams([bm for _, bm, _ in c["run"]], c["planes"], c["w"], c["h"])
    for a in m["streams"] + [m["owner"], m["ordinal"]]:
        a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def census(name: str) -> dict:
    c = case(name)
    return census_of(c["run"], c["w"], c["h"])


def story(name: str, p: int, got: np.ndarray) -> str:
    """for a failure message: where pass p's stream first differs from the model's, the workgroup and run it lies in, the owning tile and its byte"""
    c, m, cs = case(name), model(name), census(name)
    want = m["streams"][p]
    n = min(got.size, want.size)
    diff = np.flatnonzero(np.asarray(got[:n]) != want[:n])
    if not diff.size and got.size == want.size:
        return "streams equal"
    j = int(diff[0]) // 3 if diff.size else n // 3
    where = np.argwhere((m["ordinal"] == j) & ((m["owner"] >> 27) == p))
    lens = f"{got.size} bytes, the model has {want.size}"
    if not len(where):
        return f"pass {p}: {lens}; first difference at colour {j}, behind the model's last"
    ly, lx = (int(v) for v in where[0])
    key = int(m["owner"][ly, lx])
    bit, q = (key >> 2) & ((1 << 25) - 1), key & 3
    sx, sy = PASSES[p]
    r = cs["groups"][p][bit >> 13]
    return (f"pass {p} ({1 << sx}x{1 << sy}): {lens}; first difference at colour {j} = lattice point ({lx}, {ly}), corner {'TL TR BL BR'.split()[q]} of tile "
            f"{bit_tile(sx, sy, c['w'], bit)} = bit {bit}, byte {bit >> 3} = {int(c['run'][p][1][bit >> 3]):#04x}; workgroup {bit >> 13}: run of {r['tot']} colours at byte "
            f"{r['offset']} ({'LDS' if r['tot'] <= KCAP else 'direct'} path), got {np.asarray(got[3 * j: 3 * j + 3]).tolist()} want {want[3 * j: 3 * j + 3].tolist()}")
