"""TEST INFRASTRUCTURE ONLY.  Directed inputs for the gradient passes of the fused encode kernel (y2_grad_pass in yaik_amd/csrc/yk_encode2.hip;
FittingQuadSmooth, reference EncoderContext.cpp:3710-4363, restated in oracle/yaik_oracle.c:160-264).

The control flow of a pass depends on WHICH of the six acceptance variants keep a tile, WHERE the others die, how many cells the strip's viable
tiles hold and whether the curvature test killed a cell.  The images here set all of that tile by tile, without a hook in the library:

  * a TARGET tile has chosen corner values (TL is its own pixel (0, 0); TR / BL / BR are the pixels (0, 0) of the cells right of, below and
    diagonal to it, or clamped edge pixels) and an interior that is ONE variant's blend plus an error field: errors of at most rf keep that
    variant, and one pixel per other variant, where its blend differs from the kept one's, pushes that variant over rf;
  * a PLUG cell (interior 3x3 a 0 / 255 checker, row 0 constant) is alive under the curvature test but fails every tile that holds it: it
    blocks the larger tiles over a target and counts as a viable cell;
  * a DEAD cell (row 0 = c, 255, 0, c: second differences of 255 + c and 510 - c, one of them over 4 * rf + 1 for every rf <= 64) is killed by
    the curvature test: no tile over it is viable.
  Plug and dead cells leave their pixel (0, 0) free, so it can serve as a corner of the neighbouring target, and repeat it at the end of row 0
  and down column 0, which is what the clamped reads of the last tile column / row return.

variants() is the numpy model of the six tests, census() says from the oracle alone what a case really holds and which path of the kernel each
(strip, pass) takes; tests/test_gradfit_cases.py asserts on both.  A "strip" is the 64x16 pixels of one wave: 16 x 4 cells, four macro-tiles.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle.pyoracle import PASSES, OracleEncoder

VARIANTS = ("raw-O", "raw-R", "Round6-O", "Round6-R", "Round6P-O", "Round6P-R")   # O: S / 2^20, R: (S + 2^19 - 1) / 2^20
SHAPES = tuple((1 << sx, 1 << sy) for sx, sy in PASSES)                          # (TX, TY) of pass 0..6
# The two data-dependent thresholds of the kernel.  If its rule changes, this is the one place to follow it.
COMPACT_MAX_CELLS = 16                       # yk_encode2.hip, y2_grad_pass: `if (nCells <= 16) {`  (the compact path)


def curvature_limit(rf: int) -> int:
    return 4 * rf + 1                        # yk_encode2.hip, yk_encode2_kernel: `const int lim = 4 * P.rejectFactor + 1;`


def round6(v):
    r = np.asarray(v, np.int64) >> 2
    return (r << 2) | (r >> 4)


def round6p(v):
    return round6(np.minimum(np.asarray(v, np.int64) + 1, 255))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def _blends(corners, TX: int, TY: int) -> np.ndarray:
    """corners int [N, 4 (TL, TR, BL, BR), 3] -> the six blends int64 [N, 6, 3, TY, TX], in the order of VARIANTS (yaik_oracle.c:215-226)"""
    c = np.asarray(corners, np.int64)
    lF = 1024 - np.arange(TX) * (1024 // TX); rF = 1024 - lF
    tF = 1024 - np.arange(TY) * (1024 // TY); bF = 1024 - tF
    out = []
    for cs in (c, round6(c), round6p(c)):
        T = cs[:, 0, :, None] * lF + cs[:, 1, :, None] * rF                # [N, 3, TX]
        B = cs[:, 2, :, None] * lF + cs[:, 3, :, None] * rF
        S = T[:, :, None, :] * tF[:, None] + B[:, :, None, :] * bF[:, None]  # [N, 3, TY, TX]
        out += [S >> 20, (S + (1 << 19) - 1) >> 20]
    return np.stack(out, axis=1)


def _variants_many(cur, corners, TX: int, TY: int, rf: int):
    """cur int [N, 3, TY, TX] -> (ok bool [N, 6], first failing pixel in the reference's loop order ((dy * TX + dx) * 3 + channel, -1: none)
    [N, 6], number of failing pixels [N, 6])"""
    cur = np.asarray(cur, np.int64)
    fail = np.abs(cur[:, None] - _blends(corners, TX, TY)) > rf
    f = fail.transpose(0, 1, 3, 4, 2).reshape(cur.shape[0], 6, -1)
    n = f.sum(-1)
    return n == 0, np.where(n > 0, f.argmax(-1), -1), n


def _pixel(idx: int, TX: int):
    return None if idx < 0 else (int(idx % 3), int(idx // 3 % TX), int(idx // 3 // TX))


def variants(cur, corners, TX: int, TY: int, rf: int) -> dict:
    """The six tests of FittingQuadSmooth on one tile: {variant name: (passes, first failing pixel (channel, dx, dy) or None)}.
    cur: [3, TY, TX]; corners: [4, 3] = TL, TR, BL, BR per channel."""
    ok, first, _ = _variants_many(np.asarray(cur)[None], np.asarray(corners)[None], TX, TY, rf)
    return {v: (bool(ok[0, i]), _pixel(int(first[0, i]), TX)) for i, v in enumerate(VARIANTS)}


def dead_cells(planes: np.ndarray, rf: int) -> np.ndarray:
    """bool [ceil(h / 16) * 4, ceil(w / 64) * 16]: the cells the kernel's curvature test kills (row 0 of the cell, the triples 0-1-2 and 1-2-3,
    three channels, > 4 rf + 1), on the strip as the kernel stages it: rows and columns beyond the image replicate the last one, and a
    macro-tile whose origin lies outside the image is dead as a whole."""
    _, h, w = planes.shape
    H, W = (h + 15) // 16 * 16, (w + 63) // 64 * 64
    p = np.pad(np.asarray(planes, np.int64), ((0, 0), (0, H - h), (0, W - w)), mode="edge")
    r = p[:, ::4, :].reshape(3, H // 4, W // 4, 4)
    d2 = np.maximum(np.abs(r[..., 0] - 2 * r[..., 1] + r[..., 2]), np.abs(r[..., 1] - 2 * r[..., 2] + r[..., 3])).max(0)
    dead = d2 > curvature_limit(rf)
    dead[:, (w + 15) // 16 * 4:] = True
    dead[(h + 15) // 16 * 4:, :] = True
    return dead


def tile_corners(planes: np.ndarray, x: int, y: int, TX: int, TY: int) -> np.ndarray:
    """[4, 3]: the reference's clamped px() reads of a tile's corners"""
    _, h, w = planes.shape
    xs, ys = [min(x, w - 1), min(x + TX, w - 1)], [min(y, h - 1), min(y + TY, h - 1)]
    return np.array([[planes[n, yy, xx] for n in range(3)] for yy in ys for xx in xs], np.int64)


def bitmap_tiles(bitmap: np.ndarray, p: int, w: int, h: int) -> np.ndarray:
    """the swizzled bitmap of pass p (HeaderGradientTile::getSwizzleSize; yaik_oracle.c:148-198) -> bool [h / TY, w / TX]: tile accepted"""
    sx, sy = PASSES[p]
    TX, TY = SHAPES[p]
    bigX, bigY = {(3, 2): (64, 32), (2, 3): (32, 64), (2, 2): (32, 32)}.get((sx, sy), (64, 64))
    xBB, per, stepY = (w + bigX - 1) // bigX, (bigX >> sx) * (bigY >> sy), bigX >> sx
    bits = np.unpackbits(np.asarray(bitmap, np.uint8), bitorder="little")
    ty, tx = np.mgrid[0: h // TY, 0: w // TX]
    pos = ((ty * TY // bigY) * xBB + tx * TX // bigX) * per + (ty % (bigY // TY)) * stepY + tx % stepY
    return bits[pos].astype(bool)


def census(planes: np.ndarray, rf: int = 3) -> dict:
    """What an image holds, from the oracle alone (fitting_quad_smooth pass by pass, mapSmoothTile in between) plus the model:
      dead    the kernel's dead cells (dead_cells)
      paths   {(pass, strip row, strip column): (path, cells)}: "compact" (the viable tiles hold <= COMPACT_MAX_CELLS cells), "smooth" (16x16,
              no dead cell in the strip), "screened" (the rest); strips without a viable tile are not listed
      tiles   {(pass, tile y, tile x): record} of every viable tile: path, survivors (names), accepted (by the oracle), and for a tile no variant
              keeps: last = (the variant that died last in the reference's loop order, its first failing pixel)
      stray   tiles the oracle accepted although the kernel's rule calls them not viable (must be empty: the curvature test is exact)
      grad    the oracle's (count, bitmap, corner stream) of the seven passes; coverage: cells covered after them; range: (defs, nibbles, count)
              of the three planes' quantiser streams."""
    planes = np.ascontiguousarray(planes, np.int32)
    _, h, w = planes.shape
    ora = OracleEncoder(planes)
    dead = dead_cells(planes, rf)
    hc, wc = h // 4, w // 4
    cov = np.zeros((hc, wc), bool)
    paths, tiles, stray, grad = {}, {}, [], []
    for p, (sx, sy) in enumerate(PASSES):
        TX, TY = 1 << sx, 1 << sy
        NX, NY = TX // 4, TY // 4
        ny, nx = h // TY, w // TX
        res = ora.fitting_quad_smooth(sx, sy, rf)
        grad.append(res)
        after = np.zeros((hc, wc), bool)
        for n in range(3):
            after |= ora.state("mapSmoothTile", n)[::4, ::4] != 0
        if ny and nx:
            cur = planes[:, :ny * TY, :nx * TX].reshape(3, ny, TY, nx, TX).transpose(1, 3, 0, 2, 4).reshape(-1, 3, TY, TX)
            ys, xs = np.arange(ny) * TY, np.arange(nx) * TX
            Y = np.minimum(np.stack([ys, ys, ys + TY, ys + TY], -1), h - 1)            # [ny, 4]
            X = np.minimum(np.stack([xs, xs + TX, xs, xs + TX], -1), w - 1)            # [nx, 4]
            corners = planes[:, Y[:, None, :], X[None, :, :]].transpose(1, 2, 3, 0).reshape(-1, 4, 3)
            ok, first, _ = _variants_many(cur, corners, TX, TY, rf)
            ok, first = ok.reshape(ny, nx, 6), first.reshape(ny, nx, 6)
            tdead = dead[:ny * NY, :nx * NX].reshape(ny, NY, nx, NX).any((1, 3))
            viable = ~cov[:ny * NY:NY, :nx * NX:NX] & ~tdead
            accepted = after[:ny * NY:NY, :nx * NX:NX] & ~cov[:ny * NY:NY, :nx * NX:NX]
            stray += [(p, int(a), int(b)) for a, b in zip(*np.nonzero(accepted & ~viable))]
            cells = {}
            for ty, tx in zip(*np.nonzero(viable)):
                s = (int(ty) * TY // 16, int(tx) * TX // 64)
                cells[s] = cells.get(s, 0) + NX * NY
            for s, n in cells.items():
                if n <= COMPACT_MAX_CELLS:
                    path = "compact"
                elif p == 0 and not dead[4 * s[0]: 4 * s[0] + 4, 16 * s[1]: 16 * s[1] + 16].any():
                    path = "smooth"
                else:
                    path = "screened"
                paths[(p,) + s] = (path, n)
            for ty, tx in zip(*np.nonzero(viable)):
                ty, tx = int(ty), int(tx)
                surv = tuple(v for i, v in enumerate(VARIANTS) if ok[ty, tx, i])
                rec = {"path": paths[(p, ty * TY // 16, tx * TX // 64)][0], "survivors": surv, "accepted": bool(accepted[ty, tx]), "last": None}
                if not surv:
                    i = int(first[ty, tx].argmax())
                    rec["last"] = (VARIANTS[i], _pixel(int(first[ty, tx, i]), TX))
                tiles[(p, ty, tx)] = rec
        cov = after
    rng = [ora.dynamic_tile_encode(n, False)[:3] for n in range(3)]
    return {"dead": dead, "paths": paths, "tiles": tiles, "stray": stray, "grad": grad, "coverage": cov, "range": rng}


def oracle_1d(planes: np.ndarray, rf: int = 3):
    """(pix, type): the live 1-D streams of what the seven passes leave uncovered"""
    ora = OracleEncoder(np.ascontiguousarray(planes, np.int32))
    for sx, sy in PASSES:
        ora.fitting_quad_smooth(sx, sy, rf)
    for n in range(3):
        ora.dynamic_tile_compressor(n)
    return ora.streams_1d()


# ---- target tiles ------------------------------------------------------------------------------------------------------------------------------
def _tile_dead(cur, rf: int) -> bool:
    r = cur[:, ::4, :].reshape(3, -1, cur.shape[2] // 4, 4)
    d2 = np.maximum(np.abs(r[..., 0] - 2 * r[..., 1] + r[..., 2]), np.abs(r[..., 1] - 2 * r[..., 2] + r[..., 3]))
    return bool((d2 > curvature_limit(rf)).any())


def _synth(rng, corners, TX, TY, rf, want, decide=None, reject=False):
    """[3, TY, TX]: variant `want`'s blend plus the smallest errors that kill the other five, one pixel each (chosen at random among the pixels
    where the blends differ).  decide = (channel, dx, dy, sign): that pixel sits at sign * rf off the blend, or at sign * (rf + 1) with
    reject, which then is the ONLY pixel at which `want` fails.  None when the corners do not allow it."""
    B = _blends(corners[None], TX, TY)[0]
    e = np.zeros((3, TY, TX), np.int64)
    used = np.zeros((3, TY, TX), bool)
    e[:, 0, 0] = corners[0] - B[want][:, 0, 0]                             # pixel (0, 0) IS the corner TL
    used[:, 0, 0] = True
    if np.abs(e[:, 0, 0]).max() > rf:
        return None
    if decide is not None:
        ch, dx, dy, sign = decide
        e[ch, dy, dx] = sign * (rf + (1 if reject else 0))
        used[ch, dy, dx] = True
    for u in range(6):
        if u == want:
            continue
        d = B[want] - B[u]
        if decide is not None:                                             # the deciding pixel may not be what kills another variant
            hit = np.abs(e + d) > rf
            hit[decide[0], decide[2], decide[1]] = False
            if hit.any():
                continue
        elif (np.abs(e + d) > rf).any():
            continue
        cand = np.argwhere((d != 0) & ~used)
        if not len(cand):
            return None
        n, y, x = cand[rng.integers(len(cand))]
        e[n, y, x] = np.sign(d[n, y, x]) * max(rf + 1 - abs(int(d[n, y, x])), 0)
        used[n, y, x] = True
    cur = B[want] + e
    if cur.min() < 0 or cur.max() > 255 or _tile_dead(cur, rf):
        return None
    ok, first, nf = _variants_many(cur[None], corners[None], TX, TY, rf)
    alive = set(np.nonzero(ok[0])[0].tolist())
    if reject:
        ch, dx, dy, _ = decide
        if alive or nf[0, want] != 1 or first[0, want] != (dy * TX + dx) * 3 + ch:
            return None
    elif alive != {want}:
        return None
    return cur


def s_prime(corners, TX: int, TY: int) -> np.ndarray:
    """int64 [3 corner sets (raw, Round6, Round6P), 3, TY, TX]: the kernel's S' = the reference's S / 4096 (all weights are multiples of 64), so that
    blend-O = S' >> 8 and blend-R = (S' + 127) >> 8"""
    c = np.asarray(corners, np.int64)
    lF = 1024 - np.arange(TX) * (1024 // TX); rF = 1024 - lF
    tF = 1024 - np.arange(TY) * (1024 // TY); bF = 1024 - tF
    out = []
    for cs in (c, round6(c), round6p(c)):
        T = cs[0, :, None] * lF + cs[1, :, None] * rF
        B = cs[2, :, None] * lF + cs[3, :, None] * rF
        S = T[:, None, :] * tF[:, None] + B[:, None, :] * bF[:, None]
        assert not (S % 4096).any()
        out.append(S // 4096)
    return np.stack(out)


# The four ends of the kernel's windows on D = S' - 256 cur (O: -256 rf <= D <= 256 rf + 255; R: both 127 lower) as (fraction S' mod 256 of the
# deciding pixel, sign of cur - blend, rejected): D sits ON the bound in the accepted tile and ONE beyond it in the rejected one.  Only 16x16
# tiles have S' in steps of one (8-wide or 8-high tiles: steps of 2 and more), so only there a bound that is off by one can show.
WINDOW_EDGES = {"O": ((0, +1, False), (255, +1, True), (255, -1, False), (0, -1, True)),
                "R": ((129, +1, False), (128, +1, True), (128, -1, False), (129, -1, True))}


def _edge(want, frac, sign, reject):
    def factory(shape, rf):
        def make(rng, corners):
            sp = s_prime(corners, shape[0], shape[1])[want // 2]
            cand = np.argwhere(sp % 256 == frac)
            cand = cand[(cand[:, 1] != 0) | (cand[:, 2] != 0)]
            if not len(cand):
                return None
            ch, dy, dx = (int(v) for v in cand[rng.integers(len(cand))])
            dec = (ch, dx, dy, sign)
            tile = _synth(rng, corners, shape[0], shape[1], rf, want, dec, reject)
            return None if tile is None else (tile, {"decide": dec})
        return make
    return factory


def _curved(rng, corners, TX, TY, rf, ch, triple):
    """(accepted tile whose row-0 second difference is exactly 4 rf + 1 in channel ch at pixels triple .. triple + 2 of its last cell, its
    neighbour with one end of the triple one step further: 4 rf + 2, a dead cell), or None"""
    want = int(rng.integers(6))
    B = _blends(corners[None], TX, TY)[0]
    x0, y0 = TX - 4 + triple, TY - 4
    b = B[want][ch, y0, x0: x0 + 3]
    s = int(b[0] - 2 * b[1] + b[2])
    if abs(s) != 1:
        return None
    cur = B[want].copy()
    cur[ch, y0, x0: x0 + 3] += np.array([s * rf, -s * rf, s * rf])
    cur[:, 0, 0] = corners[0]
    lim = curvature_limit(rf)
    v = cur[ch, y0, x0: x0 + 3]
    if abs(int(v[0] - 2 * v[1] + v[2])) != lim or cur.min() < 0 or cur.max() > 255 or _tile_dead(cur, rf):
        return None
    if not _variants_many(cur[None], corners[None], TX, TY, rf)[0].any():
        return None
    over = cur.copy()
    over[ch, y0, x0 + 2] += s
    v = over[ch, y0, x0: x0 + 3]
    if abs(int(v[0] - 2 * v[1] + v[2])) != lim + 1 or over.min() < 0 or over.max() > 255:
        return None
    return cur, over


# ---- the canvas: strips of cells ---------------------------------------------------------------------------------------------------------------
class Canvas:
    """An image of w x h pixels, every cell DEAD unless set otherwise.  lat: pixel (0, 0) of a cell where a target fixed it."""

    def __init__(self, w: int, h: int, rf: int, seed: int):
        self.w, self.h, self.rf = w, h, rf
        self.rng = np.random.default_rng(seed)
        self.kind = np.full((h // 4, w // 4), "d", dtype="U1")
        self.lat, self.tiles, self.targets = {}, [], []

    def fill(self, cy0, cx0, ncy, ncx, kind):
        blk = self.kind[cy0: cy0 + ncy, cx0: cx0 + ncx]
        blk[blk != "t"] = kind

    def _draw(self, fixed):
        spread, lo, hi = (20, 90, 165) if self.rf > 8 else (40, 45, 210)
        have = [f for f in fixed if f is not None]
        base = np.mean(have, axis=0).astype(np.int64) if have else self.rng.integers(100, 156, 3)
        base = np.clip(base, lo + spread // 2, hi - spread // 2)
        out = np.array([f if f is not None else np.clip(base + self.rng.integers(-spread, spread + 1, 3), lo, hi) for f in fixed], np.int64)
        if fixed[0] is None and self.rf <= 1:                              # a TL that Round6 and Round6P leave alone: its low two bits repeat its top two
            out[0] = (out[0] & ~3) | (out[0] >> 6)
        return out

    def place(self, p, cy, cx, make, given=None, tries=400, **rec):
        """A target of pass p's shape with its origin at cell (cy, cx).  make(rng, corners) -> tile (or a tuple whose first item is the tile; a dict as
        its second item adds to the target's record) or None; the corners no earlier target fixed are drawn anew for every try (or taken from `given`).  Returns make's result."""
        TX, TY = SHAPES[p]
        NX, NY = TX // 4, TY // 4
        cells = [(cy, cx), (cy, cx + NX), (cy + NY, cx), (cy + NY, cx + NX)]
        assert all(y < self.h // 4 and x < self.w // 4 for y, x in cells), "a corner beyond the image: use place_ramp"
        assert (self.kind[cy: cy + NY, cx: cx + NX] != "t").all()
        fixed = [self.lat.get(c) for c in cells]
        if given is not None:
            assert all(f is None or np.array_equal(f, g) for f, g in zip(fixed, given))
            fixed = [np.asarray(g, np.int64) for g in given]
        for _ in range(tries):
            corners = self._draw(fixed)
            out = make(self.rng, corners)
            if out is not None:
                break
        else:
            return None
        for c, v in zip(cells, corners):
            self.lat[c] = v
        self.kind[cy: cy + NY, cx: cx + NX] = "t"
        self.tiles.append((4 * cy, 4 * cx, out[0] if isinstance(out, tuple) else out))
        more = out[1] if isinstance(out, tuple) and isinstance(out[1], dict) else {}
        self.targets.append(dict(rec, p=p, cy=cy, cx=cx, **more))
        return out

    def place_ramp(self, p, cy, cx, slope, level, **rec):
        """A target that is a plane A + s dx + t dy per channel, for the image's edges: the cells holding the pixels its corners read (clamped to
        the image) become plugs whose row 0 and column 0 repeat what the plane has there."""
        TX, TY = SHAPES[p]
        NX, NY = TX // 4, TY // 4
        A, (s, t) = np.asarray(self.lat.get((cy, cx), level), np.int64), slope   # an earlier target's corner, if it is one
        dy, dx = np.mgrid[0:TY, 0:TX]
        cur = A[:, None, None] + s * dx[None] + t * dy[None]
        x, y = 4 * cx, 4 * cy
        for yy, xx in ((y, x + TX), (y + TY, x), (y + TY, x + TX)):
            yy, xx = min(yy, self.h - 1), min(xx, self.w - 1)
            c = (yy // 4, xx // 4)
            if not (cy <= c[0] < cy + NY and cx <= c[1] < cx + NX):       # not a pixel of the tile itself
                v = A + s * min(xx - x, TX - 1 if xx == self.w - 1 and x + TX >= self.w else TX) + t * min(yy - y, TY - 1 if yy == self.h - 1 and y + TY >= self.h else TY)
                assert self.kind[c] != "t" and (c not in self.lat or np.array_equal(self.lat[c], v)), (p, cy, cx, c)
                self.kind[c] = "p"
                self.lat[c] = v
        self.lat[(cy, cx)] = cur[:, 0, 0]
        self.kind[cy: cy + NY, cx: cx + NX] = "t"
        self.tiles.append((y, x, cur))
        self.targets.append(dict(rec, p=p, cy=cy, cx=cx))

    def render(self) -> np.ndarray:
        img = np.zeros((3, self.h, self.w), np.int64)
        checker = (np.indices((3, 3)).sum(0) % 2) * 255
        for cy in range(self.h // 4):
            for cx in range(self.w // 4):
                k = self.kind[cy, cx]
                if k == "t":
                    continue
                c = self.lat.get((cy, cx))
                if c is None:
                    c = self.rng.integers(40, 121, 3)
                blk = np.broadcast_to(np.asarray(c)[:, None, None], (3, 4, 4)).copy()
                if k == "d":
                    blk[:, 0, 1], blk[:, 0, 2] = 255, 0
                else:
                    blk[:, 1:, 1:] = checker
                img[:, 4 * cy: 4 * cy + 4, 4 * cx: 4 * cx + 4] = blk
        for y, x, cur in self.tiles:
            img[:, y: y + cur.shape[1], x: x + cur.shape[2]] = cur
        assert img.min() >= 0 and img.max() <= 255
        return img.astype(np.int32)


# ---- strips of one (shape, path) ---------------------------------------------------------------------------------------------------------------
def _slots(p: int, path: str, row: int):
    """(macro-tiles that take a target, kind of the cells around a target, kind of the other macro-tiles of the strip).  compact: dead cells
    around, so that the targets' cells (<= 16) are all that is viable; screened / smooth: plugs, so that every cell stays viable; a screened
    16x16 strip keeps one dead macro-tile.  A 16-wide target has a free macro-tile to its right, an 8x16 one sits in the macro-tiles 0, 2 of
    even strip rows and 1, 3 of odd ones: no target's corner is another target's pixel."""
    TX, TY = SHAPES[p]
    if path == "compact":
        if (TX, TY) == (16, 16):
            return [0], "d", ["d"] * 4
        if TX == 16 or TY == 16:
            return ([0, 2] if TX == 16 or row % 2 == 0 else [1, 3]), "d", ["d"] * 4
        return [0, 1, 2, 3], "d", ["d"] * 4
    if TX == 16:
        return [0, 2], "p", ["p", "p", "p", "d" if (TY == 16 and path == "screened") else "p"]
    if TY == 16:
        return ([0, 2] if row % 2 == 0 else [1, 3]), "p", ["p"] * 4
    return [0, 1, 2, 3], "p", ["p"] * 4


def _pack(name, reqs, rf, seed, cols=4, max_rows=8):
    """reqs: [(pass, path, maker factory, record)] -> images {name_k: (Canvas, planes)}.  The requests of one (pass, path) share strips; a strip
    row of 16x16 targets is followed by a dead one (their BL / BR corners), and every image ends with a dead strip row."""
    groups = {}
    for r in reqs:
        groups.setdefault((r[0], r[1]), []).append(r)
    strips = []                                                           # (pass, path, requests)
    for (p, path), rs in groups.items():
        cap = len(_slots(p, path, 0)[0])
        strips += [(p, path, rs[i: i + cap]) for i in range(0, len(rs), cap)]
    rows, cur = [], []
    for s in strips:                                                      # a strip row holds strips of one shape class (16x16 or not)
        if cur and (len(cur) == cols or (SHAPES[cur[0][0]] == (16, 16)) != (SHAPES[s[0]] == (16, 16))):
            rows.append(cur); cur = []
        cur.append(s)
    if cur:
        rows.append(cur)
    images, k = {}, 0
    while rows:
        take, used = [], 0
        while rows and used + 2 <= max_rows:                                # a 16x16 row and its dead row, or a row and the image's closing dead row
            used += 2 if SHAPES[rows[0][0][0]] == (16, 16) else 1
            take.append(rows.pop(0))
        nrows = used + (0 if SHAPES[take[-1][0][0]] == (16, 16) else 1)
        cv = Canvas(64 * cols, 16 * nrows, rf, seed + k)
        r = 0
        for row in take:
            for col, (p, path, rs) in enumerate(row):
                mts, around, others = _slots(p, path, r)
                for m in range(4):
                    cv.fill(4 * r, 16 * col + 4 * m, 4, 4, around if m in mts else others[m])
                for m, (_, _, factory, rec) in zip(mts, rs):
                    out = cv.place(p, 4 * r, 16 * col + 4 * m, factory(SHAPES[p], rf), **dict(rec, path=path))
                    assert out is not None, (name, p, path, rec)
            r += 2 if SHAPES[row[0][0]] == (16, 16) else 1
        images[f"{name}_{k}"] = cv
        k += 1
    return images


# ---- the groups ----------------------------------------------------------------------------------------------------------------------------------
def paths_of(p: int):
    return ("compact", "screened", "smooth") if p == 0 else ("compact", "screened")


def _sole(want, decide=None, reject=False):
    return lambda shape, rf: (lambda rng, corners: _synth(rng, corners, shape[0], shape[1], rf, want, decide, reject))


def deciding_pixels(p: int, kind: str, rot: int):
    """[(variant, (channel, dx, dy, sign))]: four pixels that between them hold every row 0..3 of a cell, its first and last column, the first
    and the last cell of the tile and both signs; kind "A": a raw or Round6 variant, the channel walks 0, 1, 2; "P3": a Round6P variant with the
    pixel in channel 0 or 1 (stream 3); "P4": Round6P, channel 2 (stream 4).  Never pixel (0, 0) of the tile: that is the corner TL."""
    TX, TY = SHAPES[p]
    last = (TX - 4, TY - 4)
    base = [(0, 3, (0, 0), +1), (1, 0, last, -1), (2, 3, last, +1), (3, 0, (0, 0), -1)]      # row, column, cell, sign
    chans = {"A": (0, 1, 2, 1), "P3": (0, 1, 0, 1), "P4": (2, 2, 2, 2)}[kind]
    out = []
    for i, (row, col, cell, sign) in enumerate(base):
        v = (i + rot) % 4 if kind == "A" else 4 + (i + rot) % 2
        out.append((v, (chans[(i + rot) % 4], cell[0] + col, cell[1] + row, sign)))
    return out


def _pair_requests(p, rot=0):
    reqs = []
    for path in paths_of(p):
        for kind in ("A", "P3", "P4"):
            for v, dec in deciding_pixels(p, kind, rot + p):
                for reject in (False, True):
                    reqs.append((p, path, _sole(v, dec, reject), dict(group="B", kind=kind, variant=v, decide=dec, expect="reject" if reject else "sole")))
    return reqs


def _build_AB(p):
    reqs = [(p, path, _sole(v), dict(group="A", variant=v, expect="sole")) for path in paths_of(p) for v in range(6)]
    return _pack(f"ab{SHAPES[p][0]}x{SHAPES[p][1]}", reqs + _pair_requests(p), 3, 1000 + p)


def _build_H():
    """16x16 tiles in the three paths whose deciding pixel puts D on each end of each variant's window, and one beyond it (WINDOW_EDGES)"""
    reqs = []
    for path in paths_of(0):
        for v in range(6):
            for frac, sign, reject in WINDOW_EDGES["OR"[v % 2]]:
                reqs.append((0, path, _edge(v, frac, sign, reject), dict(group="H", variant=v, frac=frac, expect="reject" if reject else "sole")))
    return _pack("h16x16", reqs, 3, 7000)


F_PASSES, F_FACTORS = (0, 3, 6), (0, 1, 64)


def _build_F(p, rf):
    reqs = [(q, path, f, dict(rec, group="F")) for q, path, f, rec in _pair_requests(p, rot=rf)]
    return _pack(f"f{SHAPES[p][0]}x{SHAPES[p][1]}_rf{rf}", reqs, rf, 2000 + 10 * p + rf)


def _build_D_images():
    """per shape: accepted tiles whose row-0 second difference is exactly 4 rf + 1 (three channels, both triples), each followed by its
    neighbour at 4 rf + 2 (the same tile and corners, one pixel one step further: a dead cell).  One target per macro-tile (16-wide ones: every
    other macro-tile), dead cells or plugs around it in turn, every other strip row dead so that no corner is shared.  The last image ends with
    a strip row [all dead | one live cell, an accepted 4x4 tile | all dead | all dead]."""
    images = {}
    todo = [(p, ch, triple) for p in range(7) for ch in range(3) for triple in (0, 1)]
    for k, part in enumerate((todo[:14], todo[14:28], todo[28:])):
        cv = Canvas(256, 16 * 16, 3, 3000 + k)
        r, col = 0, 0                                                      # strip row, macro-tile column 0..15
        for p, ch, triple in part:
            TX, TY = SHAPES[p]
            step = 2 if TX == 16 else 1
            if col + 2 * step > 16:
                r, col = r + 2, 0
            around = "d" if (ch + triple) % 2 == 0 else "p"
            lim = curvature_limit(3)
            cv.fill(4 * r, 4 * col, 4, 4, around)
            got = cv.place(p, 4 * r, 4 * col, lambda rng, c: _curved(rng, c, TX, TY, 3, ch, triple), tries=4000, group="D", expect="accept", curve=(ch, triple, lim))
            assert got is not None, ("D", p, ch, triple)
            corners = [cv.lat[c] for c in ((4 * r, 4 * col), (4 * r, 4 * col + TX // 4), (4 * r + TY // 4, 4 * col), (4 * r + TY // 4, 4 * col + TX // 4))]
            col += step
            cv.fill(4 * r, 4 * col, 4, 4, around)
            out = cv.place(p, 4 * r, 4 * col, lambda rng, c: got[1], given=corners, group="D", expect="dead", curve=(ch, triple, lim + 1))
            assert out is not None
            col += step
        r += 2
        if k == 2:
            cv.place(6, 4 * r + 1, 16 + 5, _sole(1)(SHAPES[6], 3), group="D", expect="sole", variant=1, path="compact", lone=True)
            r += 2
        cv.h = 16 * r
        cv.kind = cv.kind[: cv.h // 4]
        images[f"d_{k}"] = cv
    return images


E_VALUES = (0, 3, 63, 64, 127, 128, 191, 192, 252, 254, 255)
E_TRIPLES = ((255, 127, 255), (127, 255, 128), (0, 255, 0), (254, 255, 0), (128, 127, 255), (255, 255, 254))


def _build_E():
    """8x8 targets whose TL is (v, v, v) for the values of E_VALUES, or one of E_TRIPLES, the other corners within +-12 of it: a Round6P variant as
    the sole survivor where the search finds one (record: expect "sole"), else a tile that every variant fails in one pixel (expect "reject");
    then the saturated D: corners and tile all 255 with one pixel 0, all 0 with one pixel 255."""
    cv = Canvas(256, 16 * 8, 3, 4000)
    slot = 0                                                               # four targets per strip, four strips per row

    def spot(path):
        nonlocal slot
        r, m = slot // 16, slot % 16
        cv.fill(4 * r, 4 * m, 4, 4, "d" if path == "compact" else "p")
        slot += 1
        return 4 * r, 4 * m

    for tl in [(v, v, v) for v in E_VALUES] + list(E_TRIPLES):
        tl = np.array(tl, np.int64)
        for want in (4, 5):
            path = "compact" if (slot // 4) % 2 == 0 else "screened"
            cy, cx = spot(path)
            done = None
            for _ in range(300):
                near = [tl] + [np.clip(tl + cv.rng.integers(-12, 13, 3), 0, 255) for _ in range(3)]
                tile = _synth(cv.rng, np.array(near), 8, 8, 3, want)
                if tile is not None:
                    done = cv.place(3, cy, cx, lambda rng, c: tile, given=near, group="E", expect="sole", variant=want, tl=tuple(int(v) for v in tl), path=path)
                    break
            if done is None:                                              # no such tile: the blend of raw-R with one pixel 11 off fails all six
                near = [tl] + [np.clip(tl + cv.rng.integers(-12, 13, 3), 0, 255) for _ in range(3)]
                tile = _blends(np.array(near)[None], 8, 8)[0][1]
                tile[1, 6, 5] += 11 if tile[1, 6, 5] < 128 else -11
                out = cv.place(3, cy, cx, lambda rng, c: tile, given=near, group="E", expect="reject", variant=want, tl=tuple(int(v) for v in tl), path=path)
                assert out is not None
    for i, (level, spike) in enumerate(((255, 0), (0, 255), (255, 0), (0, 255))):
        path = "compact" if i < 2 else "screened"
        cy, cx = spot(path)
        tile = np.full((3, 8, 8), level, np.int64)
        tile[i % 3, 2 + 4 * (i % 2), 1 + 4 * (i // 2)] = spike
        out = cv.place(3, cy, cx, lambda rng, c: tile, given=[np.full(3, level, np.int64)] * 4, group="E", expect="reject", sat=(level, spike), path=path)
        assert out is not None
    cv.h = 16 * ((slot + 15) // 16 + 1)
    cv.kind = cv.kind[: cv.h // 4]
    return {"e_0": cv}


C_COUNTS = {0: (16, 16, 32, 64, 48), 3: (12, 16, 20, 64), 6: (15, 16, 17, 64)}


def _build_C():
    """Strips whose viable tiles hold a chosen number of cells in the 16x16, 8x8 and 4x4 passes, on both sides of COMPACT_MAX_CELLS.  16x16 tiles
    come in 16 cells and 8x8 tiles in 4, so 15 and 17 exist for 4x4 only: 16x16 has 16 | 32, 8x8 has 12, 16 | 20.  The live tiles sit on a
    checkerboard (4x4, 8x8) so that no larger tile is free of dead cells; they alternate between a sole survivor (raw-R or raw-O: their TL may be
    another target's BR) and a tile that its last variant fails in one pixel.  A strip of 16 cells of 16x16 holds one tile, so there are two."""
    images = {}
    for p, counts in C_COUNTS.items():                                    # three strips per row: the fourth column holds corners only
        cv = images[f"c_{len(images)}"] = Canvas(256, 16 * 2 * ((len(counts) + 2) // 3), 3, 5000 + p)
        strip = 0
        TX, TY = SHAPES[p]
        NX, NY = TX // 4, TY // 4
        for ci, n in enumerate(counts):
            r, col = 2 * (strip // 3), strip % 3
            strip += 1
            nt = n // (NX * NY)
            if n == 64:
                cv.fill(4 * r, 16 * col, 4, 16, "p")
                spots = [(0, 4 * m) for m in range(4)] if p else [(0, 0), (0, 8)]
            elif p == 0:
                spots = [(0, 4 * m) for m in range(nt)]
                if n == 48:
                    spots = [(0, 0), (0, 8)]
                    cv.fill(4 * r, 16 * col + 4, 4, 4, "p")
            else:
                board = [(y, x) for y in range(0, 4, NY) for x in range(0, 16, NX) if (y // NY + x // NX) % 2 == 0]
                spots = board[:nt]
            for i, (y, x) in enumerate(spots):
                reject = (i + ci) % 2 == 1
                dec = (i % 3, TX - 1 - (i % 2) * (TX - 2), TY - 1 - (i % 3), 1 if i % 2 else -1)
                out = cv.place(p, 4 * r + y, 16 * col + x, _sole(i % 2, dec, reject)(SHAPES[p], 3), tries=3000, group="C", count=n, strip=(r, col),
                               variant=i % 2, decide=dec, expect="reject" if reject else "sole", path="compact" if n <= COMPACT_MAX_CELLS else ("smooth" if p == 0 and n == 64 else "screened"))
                assert out is not None, ("C", p, n, i)
    return images


G_SIZES = ((72, 24), (136, 40), (200, 136))


def _build_G(w, h, seed):
    """Targets in the last full tile column and row of an image whose sides are 8 mod 16: planes with slopes of at most 1, at levels of 200 and
    more while every other cell starts from 40..120, so that a corner read that wraps to the next row's first pixel, or a zero, is far off."""
    cv = Canvas(w, h, 3, seed)
    rng = cv.rng
    cxe, cye = w // 4, h // 4
    cv.fill(0, cxe - 2, cye, 2, "p")                                     # the half macro-tiles along both edges: plugs
    cv.fill(cye - 2, 0, 2, cxe, "p")
    right = [(2, 2), (3, 2), (4, 2), (5, 1), (6, 1)]                       # (pass, width in cells): 8x16, 8x8, 8x4, 4x8, 4x4 against the right edge
    i, k = 0, seed
    while i < h // 16:
        p, ncx = right[k % 5]
        if p == 2 and i == h // 16 - 1:                                    # the BR of an 8x16 tile is a pixel of the next strip row: keep that one free
            k += 1
            continue
        s = 0 if ncx == 1 else (1 if i % 2 else -1)
        cv.place_ramp(p, 4 * i, cxe - ncx, (s, 1 if i % 3 else -1), rng.integers(205, 235, 3), group="G", edge="right", expect="accept")
        i, k = i + (2 if p == 2 else 1), k + 1
    bottom = [(1, 2), (3, 2), (5, 2), (4, 1), (6, 1)]                      # 16x8, 8x8, 4x8, 8x4, 4x4 against the bottom edge
    for i in range(2, w // 16, 2):                                         # not under column 0: that is where a wrapped read would land
        p, ncy = bottom[(i // 2 + seed) % 5]
        t = 0 if ncy == 1 else (1 if i % 4 else -1)
        cv.place_ramp(p, cye - ncy, 4 * i, (1 if i % 3 else -1, t), rng.integers(205, 235, 3), group="G", edge="bottom", expect="accept")
    p = (3, 6, 4)[seed % 3]                                                # the corner: 8x8, 4x4 or 8x4 with all three far corners clamped
    cv.place_ramp(p, cye - SHAPES[p][1] // 4, cxe - SHAPES[p][0] // 4, (0, 0) if p == 6 else (1, -1), rng.integers(205, 235, 3), group="G", edge="corner", expect="accept")
    return cv


# ---- the case list ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _canvases() -> dict:
    out = {}
    for p in range(7):
        out.update(_build_AB(p))
    out.update(_build_C())
    out.update(_build_D_images())
    out.update(_build_E())
    for p in F_PASSES:
        for rf in F_FACTORS:
            out.update(_build_F(p, rf))
    out.update(_build_H())
    for i, (w, h) in enumerate(G_SIZES):
        out[f"g{w}x{h}"] = _build_G(w, h, 6000 + i)
    return out


def names() -> tuple:
    return tuple(_canvases())


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """{"name", "planes" int32 [3, h, w], "rf", "targets" (records: group, p, cy, cx, expect, ...), "census"}; computed once per process, never
    changed.  "<name>@rot1" / "@rot2": the same image with its channels rotated, a frame of the same shape for the batches (no targets claimed)."""
    base, _, rot = name.partition("@rot")
    cv = _canvases()[base]
    planes = cv.render() if not rot else np.ascontiguousarray(np.roll(case(base)["planes"], int(rot), axis=0))
    planes.setflags(write=False)
    return {"name": name, "planes": planes, "rf": cv.rf, "targets": () if rot else tuple(cv.targets), "census": census(planes, cv.rf)}


def target_tile(t: dict):
    """census key (pass, tile y, tile x) of a target record"""
    TX, TY = SHAPES[t["p"]]
    return t["p"], t["cy"] * 4 // TY, t["cx"] * 4 // TX


def _batches():
    """every case in a batch of three different frames of its shape and reject factor; shapes with fewer than three cases are filled up with
    channel-rotated copies, a count that is no multiple of three ends with an overlapping triple"""
    groups = {}
    for n in ALL_NAMES:
        cv = _canvases()[n]
        groups.setdefault((cv.w, cv.h, cv.rf), []).append(n)
    out = []
    for pool in groups.values():
        pool = pool + [f"{pool[0]}@rot{r}" for r in (1, 2)][: max(0, 3 - len(pool))]
        out += [tuple(pool[i: i + 3]) for i in range(0, len(pool) - 2, 3)] + ([tuple(pool[-3:])] if len(pool) % 3 else [])
    return tuple(out)


# entries of the 90 (shape, variant, path) sole-survivor classes of group A that the generator cannot place: ((TX, TY), variant name, path) -> reason
ABSENT: dict = {}

ALL_NAMES = names()
BATCHES = _batches()
C_NAMES = tuple(n for n in ALL_NAMES if n.startswith("c_"))
