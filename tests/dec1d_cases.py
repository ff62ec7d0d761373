"""TEST INFRASTRUCTURE ONLY.  Directed inputs for the 1-D range DECODE (Decompress1D, the yk_dec1d_* kernels of yk_decode.hip): '1DTL' type and
pixel streams built by hand, with values and coverage no encoder writes, and a second reference to judge the oracle with.

A case is {"name", "group", "w", "h", "range" (compressionRange), "gtil" (a tests/graddec_cases.py case with one 4x4 'GTIL' chunk, or None: it
makes the marks, one 4x4 gradient tile = one quadrant of an 8x8 tile), "plane_chunks" ([(planeBit, bitmap, stream)]: 4x4 plane-subset chunks decoded
with consistentMarks = 1 after the masks are split, so that the three planes' masks differ), "masks" (int [3, tiles]: the quadrant mask of every
8x8 tile per plane, bit 0 = top left, 1 = top right, 2 = bottom left, 3 = bottom right filled already), "color0" / "base" / "delta" (int [3, tiles],
used where the tile is coded), "L" (uint8 [3, h, w]), "typ" / "pix" (the streams handed to the decoder, cut where the case says so) and
"full_typ" / "full_pix" (whole)}.

build_streams() writes the streams in the reference's order: planes one after the other, tiles row-major, three type bytes per coded tile, and
per tile the top half then the bottom half, each half as four rows of [left quadrant 4 B][right quadrant 4 B] with absent quadrants left out; a
fully marked tile emits nothing.

model_decode() restates Decompress1D (oracle/yaik_oracle.c:yko_dec_1d) in numpy int64 on top of the gradient model's planes and
marks: per plane the offsets of a tile are the counts of the tiles before it, a coded tile reads (color0, base, delta), delta2 =
((delta * ((1 << 24) / range)) >> 8) + 1, a pixel is color0 where L == 0 and (base + (((L - 1) * delta2) >> 16)) & 255 elsewhere, bytes past the end
of either stream read as 0, marked quadrants keep their gradient pixels.  It keeps a census: "mask_at" {(mask, tile index % 4)}, "wrap" (pixels
with L >= 1 whose sum passes 255, pixels with L >= 1), "blocks" (per plane the coded tiles of every scan block of 1024 tiles), "consumed" (type
bytes, pixel bytes a whole stream holds).  defect= switches in one deliberate error; tests/test_dec1d_cases.py shows that every one of them is seen
by a named case.

Groups: a values (every delta x L, ten ranges), b byte lanes (every dword over five byte values), c quadrant masks, d scan blocks, e one tile,
f streams that end early, g per-plane masks, h batches of three.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import graddec_cases as GC

DEFECTS = ("saturate", "no_plus_one", "l_times", "l0_base", "borrow_zero", "quadrant_major", "bottom_32", "full_consumes", "planes_at_0", "block_base",
           "range_15")
VALUE_RANGES = (1, 2, 3, 7, 8, 15, 16, 17, 128, 255)
LANE_BYTES = (0, 1, 0x7F, 0x80, 0xFF)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------
def quad_masks(tile4: np.ndarray, w: int, h: int) -> np.ndarray:
    """int [planes, tiles]: the quadrant mask of every 8x8 tile, from tile4x4Mask (one plane, or three back to back)"""
    s4, tw, th = (w + 15) >> 4, w >> 3, h >> 3
    t = np.asarray(tile4, dtype=np.uint8).reshape(-1, th, s4)
    tx = np.arange(tw)
    return ((t[:, :, tx >> 1].astype(np.int64) >> ((tx & 1) * 4)) & 15).reshape(t.shape[0], -1)


def cells_of(masks1: np.ndarray, w: int) -> list:
    """[(cx, cy)] in 4x4 cells: the quadrants the masks of one plane mark"""
    tw = w >> 3
    return [(2 * (i % tw) + (k & 1), 2 * (i // tw) + (k >> 1)) for i, q in enumerate(np.asarray(masks1).tolist()) for k in range(4) if q >> k & 1]


def build_streams(w: int, h: int, masks: np.ndarray, color0: np.ndarray, base: np.ndarray, delta: np.ndarray, L: np.ndarray) -> tuple:
    """(type stream, pixel stream) of the three planes in the reference's order"""
    tw, T8 = w >> 3, (w >> 3) * (h >> 3)
    typ, pix = [], [np.zeros(0, np.uint8)]
    for p in range(3):
        for i in range(T8):
            q = int(masks[p, i])
            if q == 15:
                continue
            typ += [int(color0[p, i]), int(base[p, i]), int(delta[p, i])]
            ty, tx = divmod(i, tw)
            tile = L[p, 8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
            for half in range(2):
                for r in range(4):
                    if not q >> (2 * half) & 1:
                        pix.append(tile[4 * half + r, :4])
                    if not q >> (2 * half + 1) & 1:
                        pix.append(tile[4 * half + r, 4:])
    return np.array(typ, dtype=np.uint8), np.concatenate(pix).astype(np.uint8)


# ---- the state the 1-D call starts from: gradient pixels and marks -------------------------------------------------------------------------------
def _plane_chunks_model(w: int, h: int, chunks, planes: np.ndarray, tile4: np.ndarray) -> None:
    """DecompressGradient4x4 with planeBit 1..6 and consistentMarks = 1 (oracle/yaik_oracle.c:yko_dec_gradient_planes) onto planes [3, h, w] and the
    split tile4x4Mask [3, n]; the corner masks start empty (no RGB chunk came before)"""
    lat_w, s4 = w // 4 + 1, (w + 15) >> 4
    lat = np.zeros(((h // 4 + 1) * lat_w, 3), dtype=np.int64)
    has = np.zeros(((h // 4 + 1) * lat_w, 3), dtype=bool)
    tx4, ty4 = np.arange(4, dtype=np.int64)[None, :], np.arange(4, dtype=np.int64)[:, None]
    for m, bm, stream in chunks:
        s, rd = np.asarray(stream).tolist(), 0
        for _, tx, ty in GC.set_tiles(2, 2, w, bm):
            x, y = 4 * tx, 4 * ty
            if x >= w or y >= h:
                continue
            li = (tx + ty * lat_w, tx + ty * lat_w + 1, tx + (ty + 1) * lat_w, tx + (ty + 1) * lat_w + 1)
            for k in range(4):
                for c in range(3):
                    if m >> c & 1 and not has[li[k], c]:
                        has[li[k], c] = True
                        lat[li[k], c] = s[rd] if rd < len(s) else 0
                        rd += 1
            for c in range(3):
                if not m >> c & 1:
                    continue
                TL, TR, BL, BR = (lat[j, c] for j in li)
                Lv, Rv = TL * (4 - ty4) + BL * ty4, TR * (4 - ty4) + BR * ty4
                planes[c, y:y + 4, x:x + 4] = (Lv * (4 - tx4) + Rv * tx4) >> 4
                tile4[c, (tx >> 2) + (ty >> 1) * s4] |= 1 << ((((tx >> 1) & 1) << 2) | ((ty & 1) << 1) | (tx & 1))


def _tiled(img: np.ndarray) -> np.ndarray:
    _, h, w = img.shape
    return np.ascontiguousarray(img.reshape(3, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4).reshape(3, -1))


def gradient_state(case: dict) -> dict:
    """"planes" (uint8 [3, w h], 8x8-tiled) and "tile4" (one plane, or three once the masks are split) before the 1-D call"""
    w, h = case["w"], case["h"]
    n = ((w + 15) >> 4) * (h >> 3)
    if case["gtil"] is not None:
        g = GC.model_decode(case["gtil"])
        planes, tile4 = g["planes"].copy(), g["tile4"].copy()
    else:
        planes, tile4 = np.zeros((3, w * h), np.uint8), np.zeros(n, np.uint8)
    if case["plane_chunks"]:
        img = planes.reshape(3, h // 8, w // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(3, h, w).copy()
        t3 = np.stack([tile4] * 3)
        _plane_chunks_model(w, h, case["plane_chunks"], img, t3)
        planes, tile4 = _tiled(img), t3.reshape(-1)
    return {"planes": planes, "tile4": tile4}


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def _read(a: np.ndarray, idx: np.ndarray) -> np.ndarray:
    out = np.zeros(idx.shape, dtype=np.int64)
    ok = idx < a.size
    out[ok] = a[idx[ok]]
    return out


def _borrow_zero(Lt: np.ndarray) -> np.ndarray:
    """the bytes the borrowing zero-byte test flags, per dword of four pixels of a quadrant row"""
    b = Lt.reshape(8, 2, 4).astype(np.uint64)
    x = b[..., 0] | b[..., 1] << np.uint64(8) | b[..., 2] << np.uint64(16) | b[..., 3] << np.uint64(24)
    f = ((x - np.uint64(0x01010101)) & ~x & np.uint64(0x80808080)) & np.uint64(0xFFFFFFFF)
    return np.stack([(f >> np.uint64(8 * k + 7)) & np.uint64(1) for k in range(4)], axis=-1).astype(bool).reshape(8, 8)


def model_decode(case: dict, defect: str | None = None, typ=None, pix=None, state=None) -> dict:
    """Decompress1D over the three planes of `case` (typ= / pix= replace its streams).  Returns "planes" (uint8 [3, w h], 8x8-tiled), "tile4" (as the
    gradient phase left it: the 1-D call marks nothing) and the census (module docstring).  state= {"planes", "tile4"}: what the call starts from
    when it is not the case's own gradient phase (a parsed file: `case` then needs "w", "h", "range", "typ" and "pix" only)."""
    assert defect is None or defect in DEFECTS, defect
    w, h = case["w"], case["h"]
    T8 = (w >> 3) * (h >> 3)
    st = gradient_state(case) if state is None else state
    masks = quad_masks(st["tile4"], w, h)
    if masks.shape[0] == 1:
        masks = np.repeat(masks, 3, axis=0)
    assert state is not None or np.array_equal(masks, case["masks"]), case["name"]
    typ = np.asarray(case["typ"] if typ is None else typ, dtype=np.int64)
    pix = np.asarray(case["pix"] if pix is None else pix, dtype=np.int64)
    inv = (1 << 24) // (15 if defect == "range_15" else case["range"])
    out = st["planes"].reshape(3, T8, 8, 8).copy()
    tbase = pbase = wraps = decoded = 0
    mask_at, blocks = set(), []
    for p in range(3):
        q = masks[p]
        npix = 16 * (4 - ((q & 1) + (q >> 1 & 1) + (q >> 2 & 1) + (q >> 3 & 1)))
        ntile = np.ones(T8, np.int64) if defect == "full_consumes" else (q != 15).astype(np.int64)
        toff, poff = np.cumsum(ntile) - ntile, np.cumsum(npix) - npix
        if defect == "block_base":                                             # offsets inside the scan block of 1024 tiles only
            first = (np.arange(T8) >> 10) << 10
            toff, poff = toff - toff[first], poff - poff[first]
        tb, pb = (0, 0) if defect == "planes_at_0" else (tbase, pbase)
        blocks.append([int((q[b:b + 1024] != 15).sum()) for b in range(0, T8, 1024)])
        for i in np.flatnonzero(q != 15).tolist():
            qi = int(q[i])
            mask_at.add((qi, i & 3))
            c0, b, d = _read(typ, (tb + toff[i]) * 3 + np.arange(3)).tolist()
            d2 = ((d * inv) >> 8) + (0 if defect == "no_plus_one" else 1)
            present = np.zeros((8, 8), dtype=bool)
            Lt = np.zeros((8, 8), dtype=np.int64)
            at = pb + int(poff[i])
            for half in range(2):
                left, right = not qi >> (2 * half) & 1, not qi >> (2 * half + 1) & 1
                if half and defect == "bottom_32":
                    at = pb + int(poff[i]) + 32
                blk_present = present[4 * half:4 * half + 4]
                blk_present[:, :4], blk_present[:, 4:] = left, right
                nh = 16 * (int(left) + int(right))
                seg = _read(pix, at + np.arange(nh))
                at += nh
                blk = Lt[4 * half:4 * half + 4]
                if defect == "quadrant_major" and left and right:
                    blk[:, :4], blk[:, 4:] = seg[:16].reshape(4, 4), seg[16:].reshape(4, 4)
                else:
                    blk[blk_present] = seg                                      # row after row, left quadrant before right: the reference's loop
            v = b + (((Lt if defect == "l_times" else Lt - 1) * d2) >> 16)
            live = present & (Lt > 0)
            wraps += int((v[live] > 255).sum())
            decoded += int(live.sum())
            v = np.minimum(v, 255) if defect == "saturate" else v & 255
            zero = _borrow_zero(Lt) if defect == "borrow_zero" else Lt == 0
            v = np.where(zero, b if defect == "l0_base" else c0, v)
            out[p, i][present] = v[present]
        tbase += int((q != 15).sum())
        pbase += int(npix.sum())
    return {"planes": out.reshape(3, -1), "tile4": st["tile4"], "mask_at": mask_at, "wrap": (wraps, decoded), "blocks": blocks,
            "consumed": (3 * tbase, pbase)}


# ---- building cases ------------------------------------------------------------------------------------------------------------------------------
def _gtil(name: str, w: int, h: int, masks1: np.ndarray):
    cells = cells_of(masks1, w)
    return GC._finish(name + "_marks", "x", w, h, [("4x4", GC.bitmap_of(2, 2, w, h, cells))]) if cells else None


def _finish(name: str, group: str, w: int, h: int, rng: int, masks, color0, base, delta, L, cut=None, plane_chunks=()) -> dict:
    """masks: int [tiles] (one mask for the three planes, made by a hand-built 'GTIL' chunk) or, with plane_chunks, int [3, tiles].
    cut: {"typ": n} / {"pix": n}: the stream is cut to n bytes."""
    T8 = (w >> 3) * (h >> 3)
    masks = np.asarray(masks, dtype=np.int64)
    gt = None
    if not plane_chunks:
        gt = _gtil(name, w, h, masks)
        masks = np.stack([masks] * 3)
    bc = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int64) % 256, (3, T8)))
    L = np.ascontiguousarray(np.broadcast_to(np.asarray(L, dtype=np.int64) % 256, (3, h, w)).astype(np.uint8))
    case = {"name": name, "group": group, "w": w, "h": h, "range": rng, "gtil": gt, "plane_chunks": list(plane_chunks), "masks": masks,
            "color0": bc(color0), "base": bc(base), "delta": bc(delta), "L": L, "cut": dict(cut or {})}
    ft, fp = build_streams(w, h, masks, case["color0"], case["base"], case["delta"], L)
    case["full_typ"], case["full_pix"] = ft, fp
    case["typ"], case["pix"] = ft[:case["cut"].get("typ", ft.size)].copy(), fp[:case["cut"].get("pix", fp.size)].copy()
    for k in ("masks", "color0", "base", "delta", "L", "full_typ", "full_pix", "typ", "pix"):
        case[k].setflags(write=False)
    return case


def decodable(base: int, delta: int, rng: int) -> set:
    d2 = ((delta * ((1 << 24) // rng)) >> 8) + 1
    return {(base + (((L - 1) * d2) >> 16)) & 255 for L in range(1, 256)}


def _values(rng: int) -> dict:
    """256 x 256, nothing marked: 1024 coded tiles and 65536 pixel bytes per plane, one full scan block.  Tile t: delta = t // 4, the L of its 64
    pixels 64 (t % 4) .. + 63; base 0, 255 and (73 delta + 41) % 256 in the three planes; color0 the first value from base + 128 upwards that no L
    decodes to (base + 128 itself where every value is decodable).  Range 1: delta folded to 0 .. 127."""
    t = np.arange(1024)
    delta = (t // 4) % 128 if rng == 1 else t // 4
    base = np.stack([np.zeros(1024, np.int64), np.full(1024, 255), (73 * delta + 41) % 256])
    color0 = np.zeros((3, 1024), np.int64)
    for p in range(3):
        for d in np.unique(delta).tolist():
            sel = delta == d
            b = int(base[p, sel][0])
            dec = decodable(b, d, rng)
            color0[p, sel] = next(((b + 128 + k) % 256 for k in range(256) if (b + 128 + k) % 256 not in dec), (b + 128) % 256)
    Lt = (64 * (t % 4))[:, None] + np.arange(64)[None, :]                       # [tile, pixel of the tile row-major]
    L = Lt.reshape(32, 32, 8, 8).transpose(0, 2, 1, 3).reshape(256, 256)
    return _finish(f"values_r{rng}", "a", 256, 256, rng, np.zeros(1024, np.int64), color0, base, np.stack([delta] * 3), L)


def lane_dwords() -> np.ndarray:
    """uint8 [625, 4]: every dword over LANE_BYTES"""
    n = np.arange(625)
    return np.array(LANE_BYTES, dtype=np.uint8)[np.stack([n // 5 ** k % 5 for k in range(4)], axis=1)]


def _lanes(rng: int) -> dict:
    """64 x 40, nothing marked: 40 tiles of 16 dwords; dword j of tile i of plane p is lane_dwords()[(16 i + j + 7 p) % 625]"""
    w, h = 64, 40
    i = np.arange(40)
    dw = lane_dwords()
    L = np.zeros((3, h, w), np.int64)
    for p in range(3):
        for t in range(40):
            rows = dw[(16 * t + np.arange(16) + 7 * p) % 625].reshape(8, 8)       # row r of the tile = dwords 2 r (left) and 2 r + 1 (right)
            L[p, 8 * (t // 8):8 * (t // 8) + 8, 8 * (t % 8):8 * (t % 8) + 8] = rows
    base = np.stack([(91 * i + 17 + 50 * p) % 256 for p in range(3)])
    return _finish(f"lanes_r{rng}", "b", w, h, rng, np.zeros(40, np.int64), (base + 101) % 256, base, np.stack([(37 * i + 5 + 11 * p) % 256 for p in range(3)]), L)


def mask_formula(i: np.ndarray, shift: int = 0) -> np.ndarray:
    """every mask 0 .. 15 at every index % 4 within any 64 consecutive tiles; neighbours differ by 5"""
    return ((i >> 2) + 5 * (i & 3) + shift) & 15


def _params(w: int, h: int, seed: int = 0):
    """(color0, base, delta [3, tiles], L [3, h, w]) in which no two consecutive tiles, rows or planes repeat"""
    i = np.arange((w >> 3) * (h >> 3))
    p = np.arange(3)[:, None]
    color0, base, delta = (151 * i + 11 * p + 77 + 5 * seed) % 256, (97 * i + 31 * p + 3 + 7 * seed) % 256, (53 * i + 29 * p + 7 + 3 * seed) % 256
    y, x = np.mgrid[0:h, 0:w]
    L = np.stack([(7 * x + 13 * y + 29 * pp + 3 * (x >> 3) + 11 * seed) % 256 for pp in range(3)])
    return color0, base, delta, L


def _masks_case(name: str, group: str, rng: int = 15, shift: int = 0, seed: int = 0, cut=None, empty: bool = False) -> dict:
    w, h = 136, 72
    c = _finish(name, group, w, h, rng, mask_formula(np.arange(153), shift), *_params(w, h, seed), cut=cut)
    if empty:                                                                   # a frame of a batch that has its marks and no 1-D bytes
        c["typ"], c["pix"] = c["typ"][:0], c["pix"][:0]
        c["cut"] = {"typ": 0, "pix": 0}
    return c


def blocks_masks() -> np.ndarray:
    """520 x 264 = 65 x 33 = 2145 tiles = three scan blocks: block 0 coded whole and nothing marked (1024 tiles, 65536 pixel bytes), tiles
    1024 .. 1100 fully marked, the rest by mask_formula"""
    i = np.arange(2145)
    m = mask_formula(i)
    m[:1024] = 0
    m[1024:1101] = 15
    return m


def _blocks() -> dict:
    return _finish("blocks_520x264", "d", 520, 264, 15, blocks_masks(), *_params(520, 264, 1))


def _one_tile(w: int, q: int) -> dict:
    masks = np.array([q] if w == 8 else [q, (7 * q + 3) & 15])
    return _finish(f"tile_{w}x8_m{q}", "e", w, 8, 15, masks, *_params(w, 8, q))


def cut_points() -> dict:
    """name -> {"typ" | "pix": length}: type cuts are multiples of 3, pixel cuts of 4; of the image of masks_136x72"""
    full = case("masks_136x72")
    nt, npx = full["full_typ"].size // 3, full["full_pix"].size // 3            # per plane: the three planes share their masks
    assert nt % 3 == 0 and npx % 16 == 0
    return {"cut_typ_in0": {"typ": 150}, "cut_typ_at1": {"typ": nt}, "cut_typ_in2": {"typ": 2 * nt + 120}, "cut_typ_far": {"typ": 3 * nt - 66}, "cut_typ_0": {"typ": 0},
            "cut_pix_in0": {"pix": 404}, "cut_pix_at1": {"pix": npx}, "cut_pix_in2": {"pix": 2 * npx + 812}, "cut_pix_far": {"pix": 3 * npx - 76}, "cut_pix_0": {"pix": 0}}


CUT_NAMES = ("cut_typ_in0", "cut_typ_at1", "cut_typ_in2", "cut_typ_far", "cut_typ_0", "cut_pix_in0", "cut_pix_at1", "cut_pix_in2", "cut_pix_far", "cut_pix_0")


def _split(name: str, w: int, h: int) -> dict:
    """per-plane masks: plane p marked by mask_formula(i, 3 p + (i >> 10)), through four plane-subset 4x4 chunks with consistentMarks = 1 (planeBit 3:
    what R and G share, 1 and 2: what only R / only G has, 4: B); their streams are graddec_cases.raw_stream, fed as they are"""
    i = np.arange((w >> 3) * (h >> 3))
    masks = np.stack([mask_formula(i, 3 * p + (i >> 10)) for p in range(3)])
    sets = [set(cells_of(masks[p], w)) for p in range(3)]
    chunks = []
    for k, (m, cells) in enumerate(((3, sets[0] & sets[1]), (1, sets[0] - sets[1]), (2, sets[1] - sets[0]), (4, sets[2]))):
        assert cells
        bm = GC.bitmap_of(2, 2, w, h, sorted(cells))
        stream = GC.raw_stream(4 * len(cells) * bin(m).count("1"), k)            # no tile pops more than four corners per plane
        bm.setflags(write=False), stream.setflags(write=False)
        chunks.append((m, bm, stream))
    return _finish(name, "g", w, h, 15, masks, *_params(w, h, 2), plane_chunks=chunks)


_BUILDERS = {}
for _r in VALUE_RANGES:
    _BUILDERS[f"values_r{_r}"] = functools.partial(_values, _r)
_BUILDERS.update({
    "lanes_r15": functools.partial(_lanes, 15), "lanes_r2": functools.partial(_lanes, 2),
    "masks_136x72": lambda: _masks_case("masks_136x72", "c"),
    "blocks_520x264": _blocks,
})
for _w in (8, 16):
    for _q in range(16):
        _BUILDERS[f"tile_{_w}x8_m{_q}"] = functools.partial(_one_tile, _w, _q)
for _n in CUT_NAMES:
    _BUILDERS[_n] = (lambda n: lambda: _masks_case(n, "f", cut=cut_points()[n]))(_n)
_BUILDERS.update({
    "split_136x72": lambda: _split("split_136x72", 136, 72), "split_520x264": lambda: _split("split_520x264", 520, 264),
    # three frames of one shape: marks, parameters and streams of their own; frame 1 has its marks and both streams empty
    "batch_r15_0": lambda: _masks_case("batch_r15_0", "h", 15, 1, 3), "batch_r15_1": lambda: _masks_case("batch_r15_1", "h", 15, 6, 4, empty=True),
    "batch_r15_2": lambda: _masks_case("batch_r15_2", "h", 15, 11, 5),
    "batch_r7_0": lambda: _masks_case("batch_r7_0", "h", 7, 2, 6), "batch_r7_1": lambda: _masks_case("batch_r7_1", "h", 7, 7, 7, empty=True),
    "batch_r7_2": lambda: _masks_case("batch_r7_2", "h", 7, 12, 8),
})
BATCHES = {"batch_r15": ("batch_r15_0", "batch_r15_1", "batch_r15_2"), "batch_r7": ("batch_r7_0", "batch_r7_1", "batch_r7_2")}
ALL_NAMES = tuple(_BUILDERS)
VALUE_NAMES = tuple(f"values_r{r}" for r in VALUE_RANGES)
TILE_NAMES = tuple(n for n in ALL_NAMES if n.startswith("tile_"))
SPLIT_NAMES = ("split_136x72", "split_520x264")


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """the case, built once per process and never changed"""
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def model(name: str) -> dict:
    m = model_decode(case(name))
    m["planes"].setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle_run(name: str) -> dict:
    """OracleDecoder: the gradient chunk, split_masks, the plane-subset chunks where the case has them, then decode_1d on the case's streams zero-extended to their
    full length (decode_1d itself pads 64 bytes only); "planes", "tile4" (three planes for group g), "consumed"; computed once, never changed"""
    from oracle.pyoracle import OracleDecoder
    c = case(name)
    od = OracleDecoder(c["w"], c["h"])
    if c["gtil"] is not None:
        (sx, sy, bm, _), = c["gtil"]["chunks"]
        od.gradient(sx, sy, bm, GC.oracle_streams(c["gtil"])[0])
    od.split_masks()                                                           # Decompress1D reads every plane's own mask: the file decoder splits them before the chunk
    for m, bm, stream in c["plane_chunks"]:
        od.gradient_planes(m, bm, stream, consistent_marks=True)
    ext = lambda s, full: np.concatenate([s, np.zeros(full.size - s.size, np.uint8)])
    consumed = od.decode_1d(ext(c["typ"], c["full_typ"]), ext(c["pix"], c["full_pix"]), c["range"])
    out = {"planes": od.planes(), "tile4": od.tile4x4(bool(c["plane_chunks"])), "consumed": consumed}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def story(name: str, got_planes: np.ndarray, want_planes: np.ndarray) -> str:
    """for a failure message: the first differing plane and 8x8 tile, its mask, its parameters and where its bytes lie in the streams"""
    c = case(name)
    tw = c["w"] >> 3
    diff = np.argwhere(np.asarray(got_planes).reshape(3, -1) != np.asarray(want_planes).reshape(3, -1))
    if not diff.size:
        return "planes equal"
    p, at = int(diff[0][0]), int(diff[0][1])
    i, px = divmod(at, 64)
    q = c["masks"][p]
    before = q[:i]
    return (f"{len(diff)} bytes differ, first in plane {p}, tile {i} = ({i % tw}, {i // tw}), pixel ({px & 7}, {px >> 3}) of it: got "
            f"{int(np.asarray(got_planes).reshape(3, -1)[p, at])}, want {int(np.asarray(want_planes).reshape(3, -1)[p, at])}; mask {int(q[i]):#x}, (color0, base, delta) = "
            f"({int(c['color0'][p, i])}, {int(c['base'][p, i])}, {int(c['delta'][p, i])}), range {c['range']}, L = {int(c['L'][p, 8 * (i // tw) + (px >> 3), 8 * (i % tw) + (px & 7)])}; "
            f"coded tile {int((before != 15).sum())} of its plane, pixel offset {int(16 * (4 * i - sum(bin(int(v)).count('1') for v in before)))} in it; "
            f"streams of {c['typ'].size} / {c['pix'].size} bytes of {c['full_typ'].size} / {c['full_pix'].size}")
