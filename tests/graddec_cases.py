"""TEST INFRASTRUCTURE ONLY.  Directed inputs for the gradient DECODE (DecompressGradient16x16 .. 4x4, the kernels of yk_decode.hip): 'GTIL' chunks
built by hand, bit by bit, and a second reference to judge the oracle with.

A case is {"name", "group", "w", "h", "remap", "chunks": [(sx, sy, bitmap bytes, raw colour stream)]}.  Bitmaps are made by setting the bits of named
tiles: tile_bit() maps (shape, tile x, tile y) to the bit index in swizzle order, bit_tile() is its inverse.  Raw colour streams hold 0..250 as a file
holds them ("remap" = 250: PaletteFullRangeRemapping lies between the stream and the lattice); byte i of chunk c is (37 i + 11 + 5 c) % 251, so every
value occurs, no two consecutive triples are equal and a pop at the wrong offset always changes pixels.  A stream is as long as its chunk consumes,
less the case's shortfall.  The interpolation cases choose their corner values themselves and feed them remapped already ("remap" = 0).

model_decode() restates the seven loops sequentially, from the rule as DESIGN.md section 10 and the header of yk_decode.hip give it: tiles in bit
order; a tile with x + TX > w or y + TY > h is skipped before anything is counted; TL, TR, BL, BR are popped for the lattice points no earlier tile
of any chunk loaded; missing stream bytes read as 0; pixel = floor(bilinear numerator / (TX TY)); the tile's 4x4 cells are marked.  It also keeps
a census: per tile which corners it owned and which chunk loaded the others, the owned corners per 1024 bitmap bytes (one workgroup of
yk_decall_stream_body), which chunk overwrote which.  defect= switches in one deliberate error; tests/test_graddec_cases.py shows that every one of
them is seen by a named case.

Groups: a interpolation, b every byte pattern, c the shared bitmap word of the 16x16 pass, d the LDS cap of the colour list, e block offsets across
passes, f cross-pass state, g streams that end early, h image edges, i batches of three.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

SHAPES = {"16x16": (4, 4), "16x8": (4, 3), "8x16": (3, 4), "8x8": (3, 3), "8x4": (3, 2), "4x8": (2, 3), "4x4": (2, 2)}     # name -> (sx, sy), file order
DEFECTS = ("pop_order", "repop", "round", "earlier_wins", "edge_consumes", "remap_div", "upright")
CORNER_VALUES = (0, 1, 127, 128, 254, 255)


def shape_name(sx: int, sy: int) -> str:
    return f"{1 << sx}x{1 << sy}"


# ---- geometry: swizzle blocks of 64 pixels a side (32 along a side of 4-pixel tiles), tiles row-major inside a block, blocks row-major ---------------
def geo(sx: int, sy: int, w: int, h: int) -> dict:
    big_x, big_y = (32 if sx == 2 else 64), (32 if sy == 2 else 64)
    tpr, rows = big_x >> sx, big_y >> sy
    xbb, ybb = -(-w // big_x), -(-h // big_y)
    return {"big_x": big_x, "big_y": big_y, "tpr": tpr, "bit_count": tpr * rows, "xbb": xbb, "ybb": ybb, "nbytes": (xbb * ybb * tpr * rows) >> 3}


def tile_bit(sx: int, sy: int, w: int, tx: int, ty: int) -> int:
    """bit index of tile (tx, ty) (in tiles of this shape) of a w-wide image"""
    g = geo(sx, sy, w, 8)
    x, y = tx << sx, ty << sy
    blk = (y // g["big_y"]) * g["xbb"] + x // g["big_x"]
    return blk * g["bit_count"] + ((y % g["big_y"]) >> sy) * g["tpr"] + ((x % g["big_x"]) >> sx)


def bit_tile(sx: int, sy: int, w: int, bit: int) -> tuple:
    """(tx, ty) of a bit index: the inverse of tile_bit"""
    g = geo(sx, sy, w, 8)
    blk, t = divmod(int(bit), g["bit_count"])
    x = (blk % g["xbb"]) * g["big_x"] + ((t % g["tpr"]) << sx)
    y = (blk // g["xbb"]) * g["big_y"] + ((t // g["tpr"]) << sy)
    return x >> sx, y >> sy


def bitmap_of(sx: int, sy: int, w: int, h: int, tiles) -> np.ndarray:
    bm = np.zeros(geo(sx, sy, w, h)["nbytes"], dtype=np.uint8)
    for tx, ty in tiles:
        b = tile_bit(sx, sy, w, tx, ty)
        bm[b >> 3] |= 1 << (b & 7)
    return bm


def set_tiles(sx: int, sy: int, w: int, bitmap: np.ndarray) -> list:
    """[(bit, tx, ty)] of the set bits, ascending"""
    return [(int(b),) + bit_tile(sx, sy, w, b) for b in np.flatnonzero(np.unpackbits(np.asarray(bitmap, np.uint8), bitorder="little"))]


def raw_stream(n: int, chunk: int) -> np.ndarray:
    return ((37 * np.arange(n, dtype=np.int64) + 11 + 5 * chunk) % 251).astype(np.uint8)


def model_remap(raw: np.ndarray, rng: int, defect=None) -> np.ndarray:
    """PaletteFullRangeRemapping: v * floor((255 << 16) / range) >> 16"""
    v = np.asarray(raw, dtype=np.int64)
    if not rng:
        return v.astype(np.uint8)
    if defect == "remap_div":
        return (v * 255 // rng).astype(np.uint8)
    return ((v * ((255 << 16) // rng)) >> 16).astype(np.uint8)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(sx: int, sy: int):
    tx, ty = np.arange(1 << sx, dtype=np.int64)[None, :], np.arange(1 << sy, dtype=np.int64)[:, None]
    TX, TY = 1 << sx, 1 << sy
    return (TY - ty) * (TX - tx), (TY - ty) * tx, ty * (TX - tx), ty * tx            # TL, TR, BL, BR


def model_decode(case: dict, defect: str | None = None, render: bool = True, streams=None) -> dict:
    """The chunks of `case` one after the other.  Returns "planes" (uint8 [3, w h], 8x8-tiled), "tile4" (tile4x4Mask), "lattice" (uint8
    [(h/4+1) (w/4+1) 3]), "consumed" (bytes per chunk, missing ones included) and the census: "tiles" [(chunk, bit, tx, ty, owned corners as bits
    TL=1 TR=2 BL=4 BR=8, the chunk that loaded each of the four corners)], "skipped" [(chunk, bit)] of the set bits outside the image, "blocks"
    (per chunk: owned corners per 1024 bitmap bytes), "overlaps" {(chunk overwritten, chunk overwriting)}, "writer" / "writer_bit" (int [h/4, w/4]:
    the chunk and bit of the tile that wrote each 4x4 cell last, -1 = none).  render=False skips the pixels; streams= replaces the chunks'."""
    assert defect is None or defect in DEFECTS, defect
    w, h = case["w"], case["h"]
    lat_w, lat_h = w // 4 + 1, h // 4 + 1
    lat = np.zeros((lat_h, lat_w, 3), dtype=np.uint8)
    loader = np.full((lat_h, lat_w), -1, dtype=np.int32)
    img = np.zeros((3, h, w), dtype=np.uint8)
    writer, writer_bit = np.full((h // 4, w // 4), -1, dtype=np.int32), np.full((h // 4, w // 4), -1, dtype=np.int64)
    stride4 = (w + 15) >> 4
    tile4 = np.zeros(((stride4 << 2) * (((h + 7) >> 3) << 1)) >> 3, dtype=np.uint8)
    consumed, tiles, skipped, blocks, overlaps = [], [], [], [], set()
    for ci, (sx, sy, bitmap, raw) in enumerate(case["chunks"]):
        stream = model_remap(raw if streams is None else streams[ci], case["remap"], defect).tolist()
        TX, TY, dx, dy, sh = 1 << sx, 1 << sy, 1 << (sx - 2), 1 << (sy - 2), sx + sy
        g = geo(sx, sy, w, h)
        two_rows = g["tpr"] == 4
        W = _weights(sx, sy)
        per_block = [0] * (-(-g["nbytes"] // 1024))
        bm = np.asarray(bitmap, dtype=np.uint8)
        rd = 0
        for bit, tx, ty in set_tiles(sx, sy, w, bm):
            x, y = tx << sx, ty << sy
            if x + TX > w or y + TY > h:
                skipped.append((ci, bit))
                if defect == "edge_consumes":
                    rd += 12
                continue
            ly, lx = y >> 2, x >> 2
            pts = ((ly, lx), (ly, lx + dx), (ly + dy, lx), (ly + dy, lx + dx))
            owned = 0
            for q in ((0, 2, 1, 3) if defect == "pop_order" else (0, 1, 2, 3)):
                p = pts[q]
                again = defect == "repop"
                if defect == "upright" and q == 1 and two_rows and (bit & 7) >= 4 and (bit & 3) != 3 and (int(bm[bit >> 3]) >> ((bit & 7) - 3)) & 1:
                    again = x + 2 * TX <= w                                   # the neighbour above and to the right is a live tile
                if loader[p] < 0 or again:
                    lat[p] = [stream[rd + c] if rd + c < len(stream) else 0 for c in range(3)]
                    rd += 3
                    if loader[p] < 0:
                        loader[p] = ci
                        owned |= 1 << q
            per_block[bit >> 13] += bin(owned).count("1")
            tiles.append((ci, bit, tx, ty, owned, tuple(int(loader[p]) for p in pts)))
            cells = np.s_[y >> 2:(y + TY) >> 2, x >> 2:(x + TX) >> 2]
            before = writer[cells]
            overlaps |= {(int(v), ci) for v in np.unique(before) if v >= 0 and v != ci}
            if render:
                c4 = [lat[p].astype(np.int64)[:, None, None] for p in pts]
                num = c4[0] * W[0] + c4[1] * W[1] + c4[2] * W[2] + c4[3] * W[3]
                val = ((num + (1 << (sh - 1)) if defect == "round" else num) >> sh).astype(np.uint8)      # >> of a non-negative integer: the floor
                dst = img[:, y:y + TY, x:x + TX]
                if defect == "earlier_wins":
                    keep = np.kron(before >= 0, np.ones((4, 4), dtype=bool))
                    dst[:, ~keep] = val[:, ~keep]
                else:
                    dst[...] = val
            writer[cells], writer_bit[cells] = ci, bit
            for cy in range(y >> 2, (y + TY) >> 2):
                for cx in range(x >> 2, (x + TX) >> 2):
                    tile4[(cx >> 2) + (cy >> 1) * stride4] |= 1 << ((((cx >> 1) & 1) << 2) | ((cy & 1) << 1) | (cx & 1))
        consumed.append(rd)
        blocks.append(per_block)
    planes = img.reshape(3, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4).reshape(3, -1)
    return {"planes": np.ascontiguousarray(planes), "tile4": tile4, "lattice": lat.reshape(-1), "consumed": consumed, "tiles": tiles, "skipped": skipped,
            "blocks": blocks, "overlaps": overlaps, "writer": writer, "writer_bit": writer_bit}


# ---- building cases ------------------------------------------------------------------------------------------------------------------------------
def _lcg(n: int, mul: int, add: int) -> np.ndarray:
    """n bitmap bytes, byte k = (mul k + add) % 256: about half of the bits, no two neighbouring bytes equal"""
    return ((mul * np.arange(n, dtype=np.int64) + add) % 256).astype(np.uint8)


def _sparse(n: int, seed: int) -> np.ndarray:
    """about one bit in eight"""
    return _lcg(n, 167, 31 * seed) & _lcg(n, 91, 7 + 13 * seed) & _lcg(n, 213, 101 + seed)


def _finish(name: str, group: str, w: int, h: int, chunks, short=None, remap: int = 250, streams=None) -> dict:
    """chunks: [(shape name, bitmap)].  short: {chunk: bytes missing at the end, or "all"}.  streams: {chunk: explicit stream}."""
    assert w % 8 == 0 and h % 8 == 0
    cs = []
    for shp, bm in chunks:
        sx, sy = SHAPES[shp]
        bm = np.ascontiguousarray(bm, dtype=np.uint8)
        assert bm.size == geo(sx, sy, w, h)["nbytes"], (name, shp, bm.size)      # no bitmap is ever shorter (or longer) than its pass needs
        cs.append([sx, sy, bm, np.zeros(0, np.uint8)])
    case = {"name": name, "group": group, "w": w, "h": h, "remap": remap, "chunks": [tuple(c) for c in cs], "short": dict(short or {})}
    need = model_decode(case, render=False)["consumed"]
    for ci, c in enumerate(cs):
        if streams and ci in streams:
            c[3] = np.ascontiguousarray(streams[ci], dtype=np.uint8)
            assert c[3].size == need[ci], (name, ci, c[3].size, need[ci])
        else:
            cut = case["short"].get(ci, 0)
            n = 0 if cut == "all" else need[ci] - cut
            assert n >= 0 and (cut == 0 or need[ci] > 0), (name, ci)
            c[3] = raw_stream(n, ci)
        for a in (c[2], c[3]):
            a.setflags(write=False)
    case["chunks"] = [tuple(c) for c in cs]
    case["need"] = need
    return case


def interp_tuples() -> list:
    return list(itertools.product(CORNER_VALUES, repeat=4))                     # 1296 ordered (TL, TR, BL, BR)


def _interp(shp: str) -> dict:
    """432 isolated tiles at even tile coordinates of a 44 x 40 tile grid; tile n carries tuples 3n, 3n + 1, 3n + 2 in R, G, B"""
    sx, sy = SHAPES[shp]
    w, h = 44 << sx, 40 << sy
    tup = interp_tuples()
    where = [(2 * (n % 22), 2 * (n // 22)) for n in range(len(tup) // 3)]
    bm = bitmap_of(sx, sy, w, h, where)
    order = {bit: n for n, (bit, _, _) in enumerate(sorted((tile_bit(sx, sy, w, tx, ty), tx, ty) for tx, ty in where))}
    stream = np.zeros(12 * len(where), dtype=np.uint8)
    for n, (tx, ty) in enumerate(where):
        k = order[tile_bit(sx, sy, w, tx, ty)]                                  # the k-th tile of the scan pops the k-th twelve bytes
        for q in range(4):
            for c in range(3):
                stream[12 * k + 3 * q + c] = tup[3 * n + c][q]
    return _finish(f"interp_{shp}", "a", w, h, [(shp, bm)], remap=0, streams={0: stream})


BYTES_SIZES = {"16x16": (1024, 512), "16x8": (512, 512), "8x16": (512, 512), "8x8": (512, 256), "8x4": (256, 256), "4x8": (256, 256), "4x4": (256, 128)}


def _bytes(shp: str, kind: str) -> dict:
    w, h = BYTES_SIZES[shp]
    k = np.arange(256, dtype=np.int64)
    bm = (k if kind == "seq" else (167 * k) % 256).astype(np.uint8)
    return _finish(f"bytes_{shp}_{kind}", "b", w, h, [(shp, bm)])


def _word_halves(lo: int, hi: int) -> dict:
    """192 x 128, 16x16: three blocks a row, so bitmap word 1 holds block 2 of row 0 (its low half) and block 0 of row 1 (its high half); lo / hi:
    that half full (1) or empty (0).  The other four blocks hold a sparse pattern.  12 bitmap bytes."""
    bm = np.array([0x21, 0x84, 0x5A, 0x3C, 0, 0, 0, 0, 0x81, 0x42, 0x18, 0x24], dtype=np.uint8)
    bm[4:6] = 0xFF * lo
    bm[6:8] = 0xFF * hi
    return _finish(f"word_halves_192x128_{lo}{hi}", "c", 192, 128, [("16x16", bm)])


def _word_tail() -> dict:
    """192 x 192, 16x16: nine blocks, 18 bitmap bytes, not a multiple of 4 -- the last word of the render has two bytes behind the bitmap's end.  A
    4x4 pass before it, so that the 16x16 pass is not the first of the call."""
    bm = _lcg(18, 167, 5)
    bm[16:18] = (0xA7, 0xFF)
    return _finish("word_halves_192x192", "c", 192, 192, [("4x4", _sparse(geo(2, 2, 192, 192)["nbytes"], 3)), ("16x16", bm)])


def _full(shp: str, w: int, h: int) -> np.ndarray:
    sx, sy = SHAPES[shp]
    return np.full(geo(sx, sy, w, h)["nbytes"], 0xFF, dtype=np.uint8)


def _reuse_lattice() -> dict:
    """64 x 64: a 4x4 pass, then 15 isolated 8x8 tiles (even tile coordinates); the k-th has the corner subset k + 1 (bits TL TR BL BR) loaded already,
    each corner by a 4x4 tile of its own inside the 8x8 tile's footprint"""
    small, big = [], []
    for k in range(15):
        tx, ty = 2 * (k % 4), 2 * (k // 4)
        big.append((tx, ty))
        for q in range(4):
            if (k + 1) >> q & 1:
                small.append((2 * tx + (q & 1), 2 * ty + (q >> 1)))
    return _finish("reuse_lattice", "f", 64, 64, [("4x4", bitmap_of(2, 2, 64, 64, small)), ("8x8", bitmap_of(3, 3, 64, 64, big))])


def _overlap() -> dict:
    """64 x 64: 16x16 tile A = (0, 0), then a 4x4 and an 8x4 tile inside A -- and inside C = (2, 0), which only a LATER 16x16 chunk holds"""
    return _finish("overlap_later_wins", "f", 64, 64, [("16x16", bitmap_of(4, 4, 64, 64, [(0, 0)])), ("4x4", bitmap_of(2, 2, 64, 64, [(1, 1), (9, 2)])),
                                                     ("8x4", bitmap_of(3, 2, 64, 64, [(1, 2), (4, 0)])), ("16x16", bitmap_of(4, 4, 64, 64, [(2, 0)]))])


def _passes(name: str, group: str, w: int, h: int, order, seed: int = 0, short=None, dense=()) -> dict:
    chunks = []
    for k, shp in enumerate(order):
        n = geo(*SHAPES[shp], w, h)["nbytes"]
        chunks.append((shp, _lcg(n, 167, 29 * (seed + k)) if shp in dense else _sparse(n, seed + k)))
    return _finish(name, group, w, h, chunks, short=short)


def _corner_tiles() -> dict:
    w, h = 96, 80
    return _finish("corner_tiles", "h", w, h, [(shp, bitmap_of(sx, sy, w, h, [(0, 0), ((w >> sx) - 1, 0), (0, (h >> sy) - 1), ((w >> sx) - 1, (h >> sy) - 1)]))
                                              for shp, (sx, sy) in SHAPES.items()])


def _edge(name: str, w: int, h: int, shapes, group: str = "h") -> dict:
    """every bit of every listed pass set except in the last one, which is sparse inside the image and full outside it"""
    chunks = []
    for k, shp in enumerate(shapes):
        sx, sy = SHAPES[shp]
        bm = _full(shp, w, h)
        if k == len(shapes) - 1 and len(shapes) > 1:
            bm = _lcg(bm.size, 167, 3)
            for bit in range(bm.size * 8):
                tx, ty = bit_tile(sx, sy, w, bit)
                if ((tx + 1) << sx) > w or ((ty + 1) << sy) > h:
                    bm[bit >> 3] |= 1 << (bit & 7)
        chunks.append((shp, bm))
    return _finish(name, group, w, h, chunks)


FILE_ORDER = tuple(SHAPES)
_BUILDERS = {}
for _s in SHAPES:
    _BUILDERS[f"interp_{_s}"] = functools.partial(_interp, _s)
    _BUILDERS[f"bytes_{_s}_seq"] = functools.partial(_bytes, _s, "seq")
    _BUILDERS[f"bytes_{_s}_perm"] = functools.partial(_bytes, _s, "perm")
for _lo, _hi in ((0, 0), (0, 1), (1, 0), (1, 1)):
    _BUILDERS[f"word_halves_192x128_{_lo}{_hi}"] = functools.partial(_word_halves, _lo, _hi)
_BUILDERS.update({
    "word_halves_192x192": _word_tail,
    "cap_over_512x256": lambda: _finish("cap_over_512x256", "d", 512, 256, [("4x4", _full("4x4", 512, 256))]),
    "cap_under_496x256": lambda: _finish("cap_under_496x256", "d", 496, 256, [("4x4", _full("4x4", 496, 256))]),
    "cap_two_blocks_512x512": lambda: _finish("cap_two_blocks_512x512", "d", 512, 512, [("4x4", _full("4x4", 512, 512))]),
    "offsets_1024x512": lambda: _passes("offsets_1024x512", "e", 1024, 512, ("8x4", "4x4", "4x8"), seed=2, dense=("8x4", "4x4", "4x8")),
    "reuse_lattice": _reuse_lattice,
    "overlap_later_wins": _overlap,
    "file_order_reversed": lambda: _passes("file_order_reversed", "f", 128, 128, FILE_ORDER[::-1], seed=4),
    "eight_chunks": lambda: _passes("eight_chunks", "f", 128, 128, FILE_ORDER + ("4x4",), seed=11),
    "empty_between": lambda: _finish("empty_between", "f", 64, 64, [("8x8", _sparse(8, 1) | 1), ("16x8", np.zeros(4, np.uint8)), ("4x4", _sparse(32, 2))]),
    "single_chunk": lambda: _finish("single_chunk", "f", 64, 64, [("8x8", _lcg(8, 167, 9))]),
    "short_1": lambda: _passes("short_1", "g", 64, 64, ("16x16", "8x8", "4x4"), seed=21, short={2: 1}, dense=("4x4",)),
    "short_2": lambda: _passes("short_2", "g", 64, 64, ("16x16", "8x8", "4x4"), seed=22, short={2: 2}, dense=("4x4",)),
    "short_3": lambda: _passes("short_3", "g", 64, 64, ("16x16", "8x8", "4x4"), seed=23, short={2: 3}, dense=("4x4",)),
    "short_7": lambda: _passes("short_7", "g", 64, 64, ("16x16", "8x8", "4x4"), seed=24, short={2: 7}, dense=("4x4",)),
    "short_empty": lambda: _passes("short_empty", "g", 64, 64, ("8x8", "4x8", "4x4"), seed=25, short={1: "all"}, dense=("8x8", "4x8")),
    "edge_80x48": lambda: _edge("edge_80x48", 80, 48, ("16x16", "8x4", "4x4")),
    "edge_72x40": lambda: _edge("edge_72x40", 72, 40, ("16x16", "16x8", "8x16", "8x8", "4x4")),
    "edge_8x8": lambda: _edge("edge_8x8", 8, 8, ("16x16", "8x16", "8x8", "4x4")),
    "corner_tiles": _corner_tiles,
    # three frames of one shape and one pass list each; every frame with bitmaps, stream lengths and a shortfall of its own
    "batch_128x128_0": lambda: _passes("batch_128x128_0", "i", 128, 128, FILE_ORDER, seed=40),
    "batch_128x128_1": lambda: _passes("batch_128x128_1", "i", 128, 128, FILE_ORDER, seed=47, short={6: 5}, dense=("8x8",)),
    "batch_128x128_2": lambda: _passes("batch_128x128_2", "i", 128, 128, FILE_ORDER, seed=54, short={3: "all"}, dense=("4x4",)),
    "batch_72x40_0": lambda: _edge("batch_72x40_0", 72, 40, ("16x8", "8x8", "4x4"), "i"),
    "batch_72x40_1": lambda: _passes("batch_72x40_1", "i", 72, 40, ("16x8", "8x8", "4x4"), seed=61, short={2: 2}, dense=("4x4",)),
    "batch_72x40_2": lambda: _finish("batch_72x40_2", "i", 72, 40, [("16x8", np.zeros(8, np.uint8)), ("8x8", np.zeros(16, np.uint8)), ("4x4", _full("4x4", 72, 40))]),
    "batch_512x256_0": lambda: _finish("batch_512x256_0", "i", 512, 256, [("4x4", _full("4x4", 512, 256))], short={0: 4}),
    "batch_512x256_1": lambda: _finish("batch_512x256_1", "i", 512, 256, [("4x4", _lcg(1024, 167, 77))]),
    "batch_512x256_2": lambda: _finish("batch_512x256_2", "i", 512, 256, [("4x4", np.zeros(1024, np.uint8))]),
})
BATCHES = {"b128x128": ("batch_128x128_0", "batch_128x128_1", "batch_128x128_2"), "b72x40": ("batch_72x40_0", "batch_72x40_1", "batch_72x40_2"),
           "b512x256": ("batch_512x256_0", "batch_512x256_1", "batch_512x256_2")}
ALL_NAMES = tuple(_BUILDERS)
INTERP_NAMES = tuple(n for n in ALL_NAMES if n.startswith("interp_"))
BYTES_NAMES = tuple(n for n in ALL_NAMES if n.startswith("bytes_"))
CAP_NAMES = ("cap_over_512x256", "cap_under_496x256", "cap_two_blocks_512x512")


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """the case, built once per process and never changed"""
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def model(name: str) -> dict:
    return model_decode(case(name))


def oracle_streams(c: dict) -> list:
    """the chunks' colour streams as the oracle and the host entry point take them: after PaletteFullRangeRemapping"""
    from oracle.pyoracle import palette_remap
    return [palette_remap(raw, c["remap"]) if c["remap"] else raw for _, _, _, raw in c["chunks"]]


@functools.lru_cache(maxsize=None)
def oracle_run(name: str) -> dict:
    """OracleDecoder.gradient chunk by chunk: "planes", "tile4", "lattice" (map_rgb), "consumed"; computed once, never changed"""
    from oracle.pyoracle import OracleDecoder
    c = case(name)
    od = OracleDecoder(c["w"], c["h"])
    consumed = [od.gradient(sx, sy, bm, rgb) for (sx, sy, bm, _), rgb in zip(c["chunks"], oracle_streams(c))]
    out = {"planes": od.planes(), "tile4": od.tile4x4(), "lattice": od.map_rgb(), "consumed": consumed}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def story(name: str, got_planes: np.ndarray, want_planes: np.ndarray) -> str:
    """for a failure message: the first differing 8x8 tile, the pass and tile that wrote it last and that tile's census entry"""
    c, m = case(name), model(name)
    w = c["w"]
    diff = np.flatnonzero((np.asarray(got_planes).reshape(3, -1) != np.asarray(want_planes).reshape(3, -1)).any(axis=0))
    if not diff.size:
        return "planes equal"
    t8, px = divmod(int(diff[0]), 64)
    x, y = (t8 % (w // 8)) * 8 + (px & 7), (t8 // (w // 8)) * 8 + (px >> 3)
    ci, bit = int(m["writer"][y >> 2, x >> 2]), int(m["writer_bit"][y >> 2, x >> 2])
    if ci < 0:
        return f"8x8 tile ({t8 % (w // 8)}, {t8 // (w // 8)}), pixel ({x}, {y}): no gradient tile covers it"
    sx, sy = c["chunks"][ci][:2]
    ent = next(t for t in m["tiles"] if t[0] == ci and t[1] == bit)
    owned = [q for k, q in enumerate(("TL", "TR", "BL", "BR")) if ent[4] >> k & 1]
    others = {q: f"chunk {ent[5][k]}" for k, q in enumerate(("TL", "TR", "BL", "BR")) if not ent[4] >> k & 1}
    return (f"8x8 tile ({t8 % (w // 8)}, {t8 // (w // 8)}), pixel ({x}, {y}): written last by chunk {ci} ({shape_name(sx, sy)}) tile ({ent[2]}, {ent[3]}) = bit {bit}, "
            f"byte {bit >> 3} of its bitmap; it owned {owned or 'no corner'}, loaded by others: {others or 'none'}")
