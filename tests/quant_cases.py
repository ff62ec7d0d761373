"""TEST INFRASTRUCTURE ONLY.  Directed inputs for the 8x8 range quantiser of the fused encode kernel (the range phase of yk_encode2_kernel in
yaik_amd/csrc/yk_encode2.hip; DynamicTileEncode / GetTileDynamic_Y, restated in oracle/yaik_oracle.c:277-403).

The reference adds the terms minDiff / v of a tile's valid pixels one after the other in float and keeps mode m when err_m <= best: the later
mode wins ties.  A kernel that sums in another order must know when its own sums cannot be trusted.  This module holds

  * a numpy / exact-integer model of the stage, written against the oracle's C text (tile_model, model_streams);
  * census(): the class of every coded tile-plane of an image, from reference quantities alone;
  * TILES: 64-value literals found by the seeded search at the end of the module (python -m tests.quant_cases prints them);
  * cases(): small images that put those tiles into the contexts in which the kernel takes different paths;
  * MUTANTS: wrong pickers.  tests/test_quant_cases.py shows that each disagrees with the oracle on a committed case.

Quadrant masks: bit 0 = top-left 4x4 cell of the tile, 1 = top-right, 2 = bottom-left, 3 = bottom-right; `quads` names the VALID (coded) cells.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import pyoracle
from oracle.pyoracle import PASSES, OracleEncoder

# The one constant of the kernel this module relies on.  If the kernel's rule changes, this is the one place to follow it.
KERNEL_MARGIN = 1.00002                      # yk_encode2.hip, range phase: `near |= !(__fmul_rn(lo, 1.00002f) < hi);`
SURE_GAP = 50 * (KERNEL_MARGIN - 1.0)        # 1e-3 relative, in exact arithmetic: fifty times the kernel's margin
NEAR_GAP = 1e-6                              # class `near`: a non-zero exact gap below this (relative)
SHORTCUT_SPAN = 7                            # the split of tie_same: max - min <= 7 and > 7
LATTICE = (0, 4, 32, 36)                     # the tile's pixels that are corners of gradient tiles (pixel (0, 0) of its four cells)
ORDER_TRIALS = 10                            # arrangements of the same values census() tries for the class `order`


# ---- the model -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(mn: int, mx: int):
    """(lut int32 [6, 16], base7Bit, distance6Bit) of DynamicTile::buildTable, from the oracle"""
    lut = np.zeros(96, np.int32)
    r = pyoracle.lib().yko_build_table(int(mn), int(mx), lut.ctypes.data)
    lut = lut.reshape(6, 16)
    lut.setflags(write=False)
    return lut, r & 255, r >> 8


@functools.lru_cache(maxsize=None)
def nearest(mn: int, mx: int):
    """(minDiff int64 [6, 256], index int64 [6, 256]) of every value under the six LUTs of (mn, mx): the first nearest entry (`d < minDiff`)"""
    lut = table(mn, mx)[0].astype(np.int64)
    v = np.arange(256)
    md, ix = np.zeros((6, 256), np.int64), np.zeros((6, 256), np.int64)
    for m in range(6):
        d = np.abs(lut[m, : 16 if m < 3 else 8, None] - v[None])
        ix[m] = d.argmin(0)                                                # argmin returns the first minimum
        md[m] = d.min(0)
    md.setflags(write=False); ix.setflags(write=False)
    return md, ix


def walk(errs, start: int, strict: bool = False, first: float = 99999999.0) -> int:
    """the reference's mode walk (:361-385): the last mode with err <= best (strict: err < best, the earlier mode wins)"""
    best, mode = first, -1
    for m in range(start, 6):
        if (errs[m] < best) if strict else (errs[m] <= best):
            best, mode = errs[m], m
    return mode


def seq32(d: np.ndarray, vals: np.ndarray) -> np.ndarray:
    """float32 [6]: errorDist += (float)minDiff / (float)v over the valid pixels in row-major order, v == 0 skipped"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = d.astype(np.float32) / vals.astype(np.float32)[None]
    t[:, vals == 0] = np.float32(0)                                        # adding +0 leaves a non-negative float sum unchanged
    if t.shape[1] == 0:
        return np.zeros(6, np.float32)
    return np.add.accumulate(t, axis=1, dtype=np.float32)[:, -1]


def exact_sums(d: np.ndarray, vals: np.ndarray):
    """([6] python ints, L): the six sums as numerators over the common denominator L = lcm of the non-zero values"""
    nz = [int(v) for v in sorted(set(vals.tolist())) if v]
    L = 1
    for v in nz:
        L = L * v // math.gcd(L, v)
    w = {v: L // v for v in nz}
    return [sum(int(dd) * w[int(v)] for dd, v in zip(d[m].tolist(), vals.tolist()) if v) for m in range(6)], L


def tile_model(values, valid, start: int) -> dict:
    """One tile-plane.  values: 64 ints row-major; valid: 64 bools.  Table from the valid pixels' min / max ((0, 0) when there is none)."""
    values, valid = np.asarray(values, np.int64).ravel(), np.asarray(valid, bool).ravel()
    vals = values[valid]
    mn, mx = (int(vals.min()), int(vals.max())) if vals.size else (0, 0)
    md, ix = nearest(mn, mx)
    d, codes = md[:, vals], ix[:, vals]
    f32 = seq32(d, vals)
    num, L = exact_sums(d, vals)
    pick = walk(f32.tolist(), start)
    _, base, dist = table(mn, mx)
    return {"vals": vals, "mn": mn, "mx": mx, "d": d, "codes": codes, "f32": f32, "num": num, "L": L, "pick": pick, "exact_pick": walk(num, start, first=math.inf),
            "def": ((pick & 255) << 13 | (dist & 255) << 7 | (base & 255)) & 0xFFFF, "start": start}


def _arrangements(vals: np.ndarray, trials: int):
    yield vals[::-1]
    yield np.sort(vals)
    yield np.sort(vals)[::-1]
    rng = np.random.default_rng(int(vals.sum()) * 64 + vals.size)
    for _ in range(max(trials - 3, 0)):
        yield rng.permutation(vals)


def classify(r: dict, trials: int = ORDER_TRIALS) -> set:
    """The classes a tile-plane belongs to (a set: a tie tile can be an `order` tile too), from reference quantities alone:
      sure           every comparison of the walk is separated by SURE_GAP relative in exact arithmetic
      zero           all sums are 0
      tie_same       two compared sums are rationally equal and the two modes' minDiff agree on every valid pixel
      tie_diff       rationally equal, the minDiff differ
      near           a non-zero rational gap below NEAR_GAP relative
      close          a gap between NEAR_GAP and SURE_GAP (no class of its own in the counts)
      float_decides  the reference's pick is not the pick of exact arithmetic
      order          the reference's pick differs for another arrangement of the same values (ORDER_TRIALS arrangements are tried)
    A screening sum in another order is within 8e-6 relative of the reference's (gamma_63 plus the reciprocal's error), so it cannot
    separate the two sums of a tie_diff, near, order or float_decides tile by KERNEL_MARGIN: a kernel gets these four right only through
    its exact re-summation in the reference's order.  tie_same is right by the tie rule alone (later mode), zero needs no rule."""
    start, num = r["start"], r["num"]
    if all(n == 0 for n in num[start:]):
        return {"zero"}
    flags, b = set(), start
    for m in range(start + 1, 6):
        A, B = num[m], num[b]
        lo, hi = min(A, B), max(A, B)
        if A == B:
            flags.add("tie_same" if np.array_equal(r["d"][m], r["d"][b]) else "tie_diff")
        elif (hi - lo) < hi * NEAR_GAP:
            flags.add("near")
        elif (hi - lo) < hi * SURE_GAP:
            flags.add("close")
        if A <= B:
            b = m
    if not flags:
        return {"sure"}
    if r["pick"] != r["exact_pick"]:
        flags.add("float_decides")
    md = nearest(r["mn"], r["mx"])[0]
    for arr in _arrangements(r["vals"], trials):
        if walk(seq32(md[:, arr], arr).tolist(), start) != r["pick"]:
            flags.add("order")
            break
    return flags


PRIORITY = ("order", "float_decides", "tie_diff", "near", "tie_same", "close", "zero", "sure")


def tile_walk(w: int, h: int, bounds):
    """LeftRightOrder over the constraint box with its quirks (yaik_oracle.c:331-342): yields (x, y, rw, rh)"""
    b0, b1, b2, b3 = (int(v) for v in bounds[:4])
    cx, cy = (b0 >> 3) << 3, (b1 >> 3) << 3
    cw, ch = (((b2 + 7) >> 3) << 3) - cx, (((b3 + 7) >> 3) << 3) - cy
    x, y = cx - 8, cy
    while True:
        ok = y < cy + ch
        if ok:
            x += 8
            if x >= cx + cw:
                x, y = cx, y + 8
                ok = y < h
        rw = (x % 8) if x + 8 > cw else 8
        rh = (y % 8) if y + 8 > ch else 8
        if not ok:
            return
        yield x, y, rw, rh


def oracle_state(planes: np.ndarray, rf: int = 3):
    """(encoder after the alpha stage and the seven passes, valid bool [h, w] = mipmapMask && !smoothMap, bounds)"""
    planes = np.ascontiguousarray(planes, np.int32)
    ora = OracleEncoder(planes)
    if planes.shape[0] == 4:
        ora.mip_prefilter()
    for sx, sy in PASSES:
        ora.fitting_quad_smooth(sx, sy, rf)
    ora.dynamic_tile_encode(0, False)                                      # allocates the all-255 mask of an image without alpha
    valid = (ora.state("mipmapMask") != 0) & (ora.state("smoothMap") == 0)
    return ora, valid, ora.bounds()


def model_streams(plane: np.ndarray, valid: np.ndarray, bounds, start: int):
    """The model's tile definitions, index nibbles (packed like the reference's) and nibble count of one plane, plus per coded tile
    (x, y, tile_model record) in stream order"""
    h, w = plane.shape
    defs, codes, tiles = [], [], []
    for x, y, rw, rh in tile_walk(w, h, bounds):
        vt, pt = np.zeros((8, 8), bool), np.zeros((8, 8), np.int64)
        y1, x1 = min(y + rh, h), min(x + rw, w)
        if y1 > y and x1 > x:
            vt[: y1 - y, : x1 - x] = valid[y:y1, x:x1]
            pt[: y1 - y, : x1 - x] = plane[y:y1, x:x1]
        if not vt.any():
            continue
        r = tile_model(pt, vt, start)
        defs.append(r["def"])
        codes += r["codes"][r["pick"]].tolist()
        tiles.append((x, y, r, pt.ravel().copy(), vt.ravel().copy()))
    nib = np.zeros((len(codes) + 1) // 2, np.uint8)
    c = np.asarray(codes, np.uint8)
    nib[: (len(codes) + 1) // 2] |= c[0::2]
    nib[: len(codes) // 2] |= c[1::2] << 4
    return np.asarray(defs, np.uint16), nib, len(codes), tiles


def census(planes: np.ndarray, mode3: bool) -> dict:
    """{(plane, tile y, tile x): record} of every coded tile-plane: "flags" (classify), "cls" (the first of PRIORITY among them), "k" (its index
    in the plane's tile-definition stream), "nib0" (its first index nibble in the plane's stream), "n" (valid pixels), "quads" (mask of the cells with valid pixels), "mn", "mx", "pick" (the model's),
    "model" (tile_model record), "values" / "valid" (64 each); plus "streams": the model's (defs, nibbles, count) per plane, and "cells":
    bool [h / 4, w / 4], the cells with valid pixels.  The valid pixels come from the oracle's smoothMap and mipmapMask.
    By the kernel's own error bound (a screening sum within 8e-6 relative of the reference's, KERNEL_MARGIN = 2e-5 between two sums it trusts) a
    kernel can get the classes order, float_decides, tie_diff and near right only through its exact path: see classify()."""
    planes = np.ascontiguousarray(planes, np.int32)
    _, valid, bounds = oracle_state(planes)
    out, streams = {}, []
    for p in range(3):
        defs, nib, nn, tiles = model_streams(planes[p], valid, bounds, 3 if mode3 else 0)
        streams.append((defs, nib, nn))
        at = 0
        for k, (x, y, r, values, vt) in enumerate(tiles):
            flags = classify(r)
            q = vt.reshape(2, 4, 2, 4).any((1, 3)).ravel()
            out[(p, y // 8, x // 8)] = {"flags": flags, "cls": next(c for c in PRIORITY if c in flags), "k": k, "n": int(vt.sum()),
                                        "quads": int(sum(1 << i for i in range(4) if q[i])), "mn": r["mn"], "mx": r["mx"], "pick": r["pick"],
                                        "model": r, "values": values, "valid": vt, "nib0": at}
            at += int(vt.sum())
    h, w = valid.shape
    return {"tiles": out, "streams": streams, "cells": valid.reshape(h // 4, 4, w // 4, 4).any((1, 3)), "bounds": np.asarray(bounds)}


# ---- wrong pickers -------------------------------------------------------------------------------------------------------------------------------
def tree32(d: np.ndarray, vals: np.ndarray) -> np.ndarray:
    """float32 [6]: the same terms added pairwise (a binary tree over the valid pixels in row-major order)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = d.astype(np.float32) / vals.astype(np.float32)[None]
    t[:, vals == 0] = np.float32(0)
    n = 1
    while n < t.shape[1]:
        n *= 2
    t = np.concatenate([t, np.zeros((6, n - t.shape[1]), np.float32)], axis=1)
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


def kernel_rule(rec: dict, wide: bool = False, ignore_diff: bool = False) -> int:
    """A picker built like the kernel's rule: tree-order screening sums decide what KERNEL_MARGIN separates; an exact tie of the screening sums
    is the later mode's when the two modes' minDiff agree for every value from min to min + 7 and max - min <= 7; everything else is
    the reference's own pick (the exact path).  wide: the span test left out; ignore_diff: the row comparison left out."""
    r = rec["model"]
    start, mn, mx = r["start"], r["mn"], r["mx"]
    T = tree32(r["d"], r["vals"])
    md = nearest(mn, mx)[0]
    bm, bt, amb = start, T[start], False
    for m in range(start + 1, 6):
        t = T[m]
        lo, hi = min(t, bt), max(t, bt)
        if t == bt:
            if t != 0:
                rows = slice(mn, min(mn + 7, mx) + 1)
                same = ignore_diff or np.array_equal(md[m, rows], md[bm, rows])
                if (mx - mn > SHORTCUT_SPAN and not wide) or not same:
                    amb = True
        elif not (np.float32(lo) * np.float32(KERNEL_MARGIN) < hi):
            amb = True
        if t <= bt:
            bm = m
        bt = lo
    return r["pick"] if amb else bm


def _def_of(mode: int, mn: int, mx: int) -> int:
    _, base, dist = table(mn, mx)
    return ((mode & 255) << 13 | (dist & 255) << 7 | (base & 255)) & 0xFFFF


def _mut_all_pixels(rec):
    """min / max over all 64 pixels of the tile instead of the valid ones"""
    values, valid, start = rec["values"], rec["valid"], rec["model"]["start"]
    mn, mx = int(values.min()), int(values.max())
    vals = values[valid]
    return _def_of(walk(seq32(nearest(mn, mx)[0][:, vals], vals).tolist(), start), mn, mx)


def _mut_zeros(rec):
    """terms of v == 0 added like any other: minDiff / 0 is inf or nan"""
    r = rec["model"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = r["d"].astype(np.float32) / r["vals"].astype(np.float32)[None]
        f = np.add.accumulate(t, axis=1, dtype=np.float32)[:, -1]
    return _def_of(walk(f.tolist(), r["start"]), r["mn"], r["mx"])


def _simple(fn):
    return lambda rec: _def_of(fn(rec["model"]), rec["model"]["mn"], rec["model"]["mx"])


MUTANTS = {
    "tree-order float32 sum": _simple(lambda r: walk(tree32(r["d"], r["vals"]).tolist(), r["start"])),
    "float64 sum": _simple(lambda r: walk([sum_f64(r, m) for m in range(6)], r["start"])),
    "exact-arithmetic pick": _simple(lambda r: r["exact_pick"]),
    "< instead of <=": _simple(lambda r: walk(r["f32"].tolist(), r["start"], strict=True)),
    "tie shortcut at max - min > 7": lambda rec: _def_of(kernel_rule(rec, wide=True), rec["model"]["mn"], rec["model"]["mx"]),
    "tie shortcut although minDiff differ": lambda rec: _def_of(kernel_rule(rec, ignore_diff=True), rec["model"]["mn"], rec["model"]["mx"]),
    "min / max over all 64 pixels": _mut_all_pixels,
    "zeros not skipped": _mut_zeros,
}


def sum_f64(r: dict, m: int) -> float:
    s = 0.0
    for dd, v in zip(r["d"][m].tolist(), r["vals"].tolist()):
        if v:
            s += dd / v
    return s


# ---- the tiles -----------------------------------------------------------------------------------------------------------------------------------
# Printed by the search at the end of this module (seed 20261021; it met every count it asked for within a minute of CPU):
#   ties: 3699 multisets tried, found {'shortcut_wide': 2, 'shortcut_diff': 2, 'order0': 3, 'order3': 3, 'float_decides': 6, 'tie_diff': 6}, partial {14: 1, 13: 1, 11: 1, 7: 1, 6: 1, 9: 1, 3: 1, 12: 1, 5: 1, 10: 1, 8: 1, 1: 1}
#   near: 879 triples tried, found 3
# quads: the valid cells the class holds for (the other cells hold the value the gradient tiles cover them with); start: the start mode it holds
# for; flag: the class the search built the tile for (census() must find it: tests/test_quant_cases.py).  The commonest value sits on the
# lattice pixels, so a tile can stand in a flat surround of that value.  order_*a / order_*b: two arrangements of the same 64 values
# for which the reference picks different modes.  shortcut_*: tie_diff tiles whose pairwise float32 sums tie exactly as well while the
# reference's pick is the EARLIER mode: what a tie shortcut taken once too often gets wrong.
TILES = {
    "float_decides_0": dict(quads=15, start=3, flag="float_decides", v=(78, 76, 76, 76, 78, 76, 76, 76, 76, 76, 76, 76, 76, 76, 76, 76, 76, 76, 76, 76, 76, 82, 75, 75, 75, 75, 75, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78)),
    "tie_diff_0": dict(quads=15, start=3, flag="tie_diff", v=(196, 147, 147, 147, 196, 147, 147, 147, 225, 225, 225, 225, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 12, 12, 12, 12, 12, 12, 12, 196, 12, 12, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196)),
    "float_decides_1": dict(quads=15, start=0, flag="float_decides", v=(55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 13, 13, 131, 131, 131, 131, 131, 11, 11, 55, 11, 11, 11, 55, 11, 11, 11, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88, 88)),
    "float_decides_2": dict(quads=15, start=3, flag="float_decides", v=(41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 48, 57, 57, 25, 25, 25, 25, 25, 25, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28)),
    "tie_diff_1": dict(quads=15, start=3, flag="tie_diff", v=(32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 29, 29, 32, 29, 29, 29, 32, 35, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30)),
    "part7_tie_diff": dict(quads=7, start=3, flag="tie_diff", v=(25, 30, 30, 30, 25, 30, 30, 57, 57, 57, 57, 57, 57, 57, 57, 57, 57, 57, 57, 57, 57, 57, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 42, 42, 42, 25, 25, 25, 25, 42, 42, 42, 42, 25, 25, 25, 25)),
    "tie_diff_2": dict(quads=15, start=3, flag="tie_diff", v=(68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 68, 60, 60, 74, 68, 74, 74, 74, 74, 74, 74, 74, 74, 74, 74, 74, 74, 42, 42, 42, 42, 44, 44, 44, 44, 44, 44, 44, 44, 44, 44, 44)),
    "part10_tie_diff": dict(quads=10, start=3, flag="tie_diff", v=(14, 14, 14, 14, 14, 12, 12, 12, 14, 14, 14, 14, 12, 12, 12, 11, 14, 14, 14, 14, 11, 21, 21, 9, 14, 14, 14, 14, 9, 9, 9, 9, 14, 14, 14, 14, 14, 9, 9, 9, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14)),
    "tie_diff_3": dict(quads=15, start=3, flag="tie_diff", v=(27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 41, 41, 41, 41, 41, 41, 41, 27, 41, 9, 9, 27, 9, 9, 9, 9, 9, 9, 9, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20)),
    "tie_diff_4": dict(quads=15, start=3, flag="tie_diff", v=(30, 26, 26, 26, 30, 26, 26, 26, 26, 26, 26, 26, 26, 26, 26, 136, 16, 16, 16, 16, 16, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30)),
    "float_decides_3": dict(quads=15, start=0, flag="float_decides", v=(200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 204, 204, 172, 172, 200, 172, 172, 172, 200, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180)),
    "tie_diff_5": dict(quads=15, start=3, flag="tie_diff", v=(132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 132, 153, 153, 153, 153, 153, 153, 153, 132, 153, 153, 153, 132, 153, 153, 153, 153, 153, 153, 153, 153, 153, 153, 153, 214, 214, 214, 214, 94, 94, 94, 94, 176, 176, 176, 176, 176, 176, 176, 176)),
    "part12_tie_diff": dict(quads=12, start=3, flag="tie_diff", v=(135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 140, 140, 140, 135, 140, 140, 140, 140, 140, 217, 97, 97, 97, 97, 97, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135)),
    "part6_tie_diff": dict(quads=6, start=3, flag="tie_diff", v=(72, 72, 72, 72, 72, 60, 60, 60, 72, 72, 72, 72, 60, 60, 60, 60, 72, 72, 72, 72, 60, 60, 60, 236, 72, 72, 72, 72, 13, 13, 13, 13, 72, 13, 13, 13, 72, 72, 72, 72, 13, 13, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72)),
    "order_s3_0a": dict(quads=15, start=3, flag="order", v=(7, 5, 5, 5, 7, 5, 5, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 10, 10, 4, 7, 4, 4, 4, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7)),
    "order_s3_0b": dict(quads=15, start=3, flag="order", v=(7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 4, 4, 4, 4, 10, 10, 7, 6, 6, 6, 7, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5)),
    "shortcut_wide_0": dict(quads=15, start=3, flag="tie_diff", v=(216, 251, 216, 128, 216, 28, 28, 128, 250, 28, 216, 250, 128, 216, 128, 128, 216, 250, 216, 250, 128, 251, 216, 251, 251, 250, 128, 250, 128, 28, 28, 28, 216, 28, 28, 250, 216, 128, 216, 216, 250, 128, 216, 128, 216, 251, 250, 28, 216, 216, 128, 216, 216, 128, 128, 28, 28, 128, 250, 251, 251, 251, 28, 128)),
    "order_s3_1a": dict(quads=15, start=3, flag="order", v=(156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 214, 215, 95, 95, 95, 95, 108, 108, 108, 108, 108, 108)),
    "order_s3_1b": dict(quads=15, start=3, flag="order", v=(156, 108, 108, 108, 156, 108, 108, 108, 95, 95, 95, 95, 215, 214, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156)),
    "part3_tie_diff": dict(quads=3, start=3, flag="tie_diff", v=(12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 14, 14, 14, 14, 15, 8, 8, 8, 8, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12)),
    "float_decides_4": dict(quads=15, start=3, flag="float_decides", v=(50, 38, 38, 38, 50, 38, 38, 38, 38, 38, 38, 38, 38, 38, 38, 38, 38, 38, 38, 38, 38, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 50, 234, 234, 234, 50, 234, 234, 234, 226, 226, 226, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50)),
    "order_s3_2a": dict(quads=15, start=3, flag="order", v=(47, 35, 35, 35, 47, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 53, 21, 21, 21, 21, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25)),
    "order_s3_2b": dict(quads=15, start=3, flag="order", v=(47, 25, 25, 25, 47, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 21, 21, 21, 21, 53, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35, 35)),
    "float_decides_5": dict(quads=15, start=3, flag="float_decides", v=(66, 60, 60, 60, 66, 60, 60, 60, 60, 60, 60, 60, 60, 60, 60, 60, 60, 60, 60, 60, 60, 60, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 66, 27, 147, 147, 66, 147, 147, 147, 147, 147, 147, 147, 147, 147, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66, 66)),
    "shortcut_diff_0": dict(quads=15, start=0, flag="tie_diff", v=(17, 19, 19, 19, 17, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 19, 22, 22, 22, 22, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18)),
    "part9_tie_diff": dict(quads=9, start=3, flag="tie_diff", v=(23, 14, 14, 14, 23, 23, 23, 23, 14, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 63, 23, 23, 23, 23, 3, 3, 3, 3, 23, 23, 23, 23, 3, 3, 42, 42, 23, 23, 23, 23, 42, 42, 42, 42)),
    "part13_tie_diff": dict(quads=13, start=0, flag="tie_diff", v=(165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 168, 168, 168, 165, 165, 165, 165, 165, 168, 168, 168, 165, 168, 168, 168, 168, 168, 168, 168, 168, 136, 136, 136, 136, 136, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154)),
    "part14_tie_diff": dict(quads=14, start=0, flag="tie_diff", v=(32, 32, 32, 32, 32, 66, 66, 66, 32, 32, 32, 32, 66, 66, 66, 66, 32, 32, 32, 32, 66, 66, 66, 66, 32, 32, 32, 32, 138, 138, 138, 138, 32, 138, 152, 152, 32, 152, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72, 72)),
    "shortcut_diff_1": dict(quads=15, start=0, flag="tie_diff", v=(5, 4, 4, 4, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 5, 3, 3, 3, 5, 3, 3, 3, 3, 3, 3, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5)),
    "order_s0_0a": dict(quads=15, start=0, flag="order", v=(69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 34, 34, 153, 153, 153, 153, 153, 153, 153, 153, 153, 69, 153, 153, 153, 69, 153, 33, 33, 33, 33, 33, 33, 33, 33, 33, 33, 33, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135)),
    "order_s0_0b": dict(quads=15, start=0, flag="order", v=(69, 135, 135, 135, 69, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 135, 33, 33, 33, 33, 33, 33, 33, 33, 33, 33, 33, 153, 153, 153, 153, 69, 153, 153, 153, 69, 153, 153, 153, 153, 153, 153, 34, 34, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69, 69)),
    "part11_tie_diff": dict(quads=11, start=3, flag="tie_diff", v=(11, 9, 9, 9, 11, 9, 9, 9, 9, 9, 9, 14, 14, 14, 14, 14, 14, 14, 14, 14, 8, 8, 8, 8, 8, 8, 8, 8, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11)),
    "order_s0_1a": dict(quads=15, start=0, flag="order", v=(165, 121, 121, 121, 165, 121, 121, 121, 121, 121, 121, 121, 121, 234, 234, 234, 234, 234, 234, 234, 114, 114, 114, 114, 114, 114, 114, 114, 114, 114, 114, 114, 165, 114, 114, 114, 165, 114, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165)),
    "order_s0_1b": dict(quads=15, start=0, flag="order", v=(165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 114, 114, 114, 114, 165, 114, 114, 114, 165, 114, 114, 114, 114, 114, 114, 114, 114, 114, 234, 234, 234, 234, 234, 234, 234, 121, 121, 121, 121, 121, 121, 121, 121, 121, 121, 121)),
    "part5_tie_diff": dict(quads=5, start=0, flag="tie_diff", v=(7, 9, 9, 9, 7, 7, 7, 7, 9, 9, 9, 9, 7, 7, 7, 7, 9, 9, 14, 14, 7, 7, 7, 7, 14, 14, 14, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 7, 7, 7, 7, 8, 8, 8, 8, 7, 7, 7, 7)),
    "shortcut_wide_1": dict(quads=15, start=3, flag="tie_diff", v=(189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 14, 14, 14, 14, 14, 14, 14, 189, 14, 237, 237, 189, 237, 237, 237, 237, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 63, 63, 63, 63, 63, 63, 63, 63, 63)),
    "part1_tie_diff": dict(quads=1, start=3, flag="tie_diff", v=(15, 15, 15, 15, 15, 15, 15, 15, 15, 23, 23, 23, 15, 15, 15, 15, 23, 23, 65, 5, 15, 15, 15, 15, 5, 5, 5, 6, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15)),
    "order_s0_2a": dict(quads=15, start=0, flag="order", v=(198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 212, 212, 212, 212, 152, 152, 152, 198, 152, 152, 152, 198, 152, 152, 152, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176)),
    "order_s0_2b": dict(quads=15, start=0, flag="order", v=(198, 176, 176, 176, 198, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 152, 152, 152, 152, 152, 152, 198, 152, 152, 152, 198, 212, 212, 212, 212, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198)),
    "part8_tie_diff": dict(quads=8, start=3, flag="tie_diff", v=(63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 123, 125, 5, 63, 63, 63, 63, 5, 5, 5, 21)),
    "near_0": dict(quads=15, start=3, flag="near", v=(144, 172, 172, 172, 144, 172, 172, 172, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 204, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 144, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175)),
    "near_1": dict(quads=15, start=3, flag="near", v=(18, 146, 146, 146, 18, 146, 146, 146, 146, 146, 146, 146, 146, 146, 146, 146, 146, 182, 182, 182, 198, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 141, 141, 141, 141, 141, 141, 141, 141, 141, 141, 141)),
    "near_2": dict(quads=15, start=0, flag="near", v=(23, 213, 213, 213, 23, 213, 213, 102, 102, 102, 102, 102, 102, 102, 246, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 140, 140, 140, 140, 140, 140, 140, 140, 140, 140, 140)),
}
# ---- end of the tiles


# ---- the search (python -m tests.quant_cases [seconds]): prints the literals of TILES ----------------------------------------------------------------
QUADS_OF_PIXEL = np.array([(i // 32) * 2 + (i % 8) // 4 for i in range(64)])


def valid_of(quads: int) -> np.ndarray:
    return ((quads >> QUADS_OF_PIXEL) & 1).astype(bool)


def arrange(rest, quads: int, c: int, cover=None) -> np.ndarray:
    """64 values: c on the lattice pixels of the valid cells, `rest` on their other pixels in row-major order, `cover` (default c) on the others"""
    valid = valid_of(quads)
    out = np.full(64, c if cover is None else cover, np.int64)
    free = [i for i in range(64) if valid[i] and i not in LATTICE]
    assert len(rest) == len(free), (len(rest), len(free))
    out[[i for i in LATTICE if valid[i]]] = c
    out[free] = rest
    return out


def _rec(values, quads, start):
    valid = valid_of(quads)
    return {"model": tile_model(values, valid, start), "values": np.asarray(values, np.int64), "valid": valid}


def _tie_multiset(rng, N, start, span=None):
    """a directed tie: two modes a < b, two values whose minDiff differences cancel (n1 d1 / v1 = n2 d2 / v2), the rest of the N pixels on
    values on which the two modes agree.  Returns (counts {value: n}, v1, v2) or None."""
    span = int(rng.choice([5, 6, 7, 7, 12, 20, 32, 60, 120, 223])) if span is None else span
    mn = int(rng.integers(1, max(2, min(224, 256 - span))))
    mx = min(mn + span, 255)
    md = nearest(mn, mx)[0]
    a, b = sorted(rng.choice(np.arange(start, 6), 2, replace=False).tolist())
    dl = md[a] - md[b]
    if dl[mn] or dl[mx]:
        return None
    pos = [v for v in range(mn + 1, mx) if dl[v] > 0]
    neg = [v for v in range(mn + 1, mx) if dl[v] < 0]
    if not pos or not neg:
        return None
    v1, v2 = int(rng.choice(pos)), int(rng.choice(neg))
    p, q = int(-dl[v2]) * v1, int(dl[v1]) * v2
    g = math.gcd(p, q)
    p, q = p // g, q // g
    if p + q > N - 6:
        return None
    t = int(rng.integers(1, (N - 6) // (p + q) + 1))
    counts = {v1: p * t, v2: q * t}
    rest = N - (p + q) * t
    same = [v for v in range(mn + 1, mx) if dl[v] == 0]
    n3 = int(rng.integers(0, rest - 4)) if same and rest > 5 and rng.random() < 0.6 else 0
    if n3:
        v3 = int(rng.choice(same))
        counts[v3] = counts.get(v3, 0) + n3
    rest -= n3
    nmx = int(rng.integers(1, max(2, rest - 3)))
    counts[mx] = counts.get(mx, 0) + nmx
    counts[mn] = counts.get(mn, 0) + rest - nmx
    return counts, v1, v2


def _layouts(rng, counts, quads, v1, v2, n):
    """arrangements of a multiset with the commonest value on the lattice: the two values of the tie at opposite ends, then shuffles"""
    nl = sum(1 for i in LATTICE if valid_of(quads)[i])
    c = max(counts, key=lambda v: counts[v])
    if counts[c] < nl:
        return
    cnt = dict(counts)
    cnt[c] -= nl
    mid = [v for v in cnt if v not in (v1, v2) for _ in range(cnt[v])]
    block = [v1] * cnt.get(v1, 0) + mid + [v2] * cnt.get(v2, 0)
    yield arrange(block, quads, c)
    yield arrange(block[::-1], quads, c)
    for _ in range(n):
        yield arrange(rng.permutation(block), quads, c)


def _near_multiset(rng, start):
    """three values whose minDiff differences nearly cancel: the smallest non-zero |n1 d1 / v1 + n2 d2 / v2 + n3 d3 / v3| over a grid of counts"""
    span = int(rng.choice([60, 120, 180, 223]))
    mn = int(rng.integers(1, 256 - span))
    mx = mn + span
    md = nearest(mn, mx)[0]
    a, b = sorted(rng.choice(np.arange(start, 6), 2, replace=False).tolist())
    dl = md[a] - md[b]
    if dl[mn] or dl[mx]:
        return None
    nzv = [v for v in range(max(mn + 1, 100), mx) if dl[v]]
    if len(nzv) < 3:
        return None
    v = [int(x) for x in rng.choice(nzv, 3, replace=False)]
    if len({np.sign(dl[x]) for x in v}) < 2:
        return None
    n = np.arange(1, 21)
    X = (n[:, None, None] * int(dl[v[0]]) * v[1] * v[2] + n[None, :, None] * int(dl[v[1]]) * v[0] * v[2] + n[None, None, :] * int(dl[v[2]]) * v[0] * v[1])
    A = np.abs(X)
    A[A == 0] = np.iinfo(np.int64).max
    i = np.unravel_index(A.argmin(), A.shape)
    if A[i] * 1e6 > 4 * v[0] * v[1] * v[2] or n[i[0]] + n[i[1]] + n[i[2]] > 56:
        return None
    counts = {v[0]: int(n[i[0]]), v[1]: int(n[i[1]]), v[2]: int(n[i[2]])}
    rest = 64 - sum(counts.values())
    counts[mx] = 1
    counts[mn] = rest - 1
    return counts, v[0], v[1]


def _lit(name, values, quads, start, flag):
    v = ", ".join(str(int(x)) for x in values)
    return f'    "{name}": dict(quads={quads}, start={start}, flag="{flag}", v=({v})),'


def _search(seconds: float, seed: int = 20261021):
    """Every tie multiset goes to ONE class (the one still furthest from its count), so the committed tiles of different classes differ."""
    import time
    rng = np.random.default_rng(seed)
    t_end = time.time() + seconds
    want = {"shortcut_wide": 2, "shortcut_diff": 2, "order0": 3, "order3": 3, "float_decides": 6, "tie_diff": 6}
    partial = (14, 13, 11, 7, 6, 9, 3, 12, 5, 10, 8, 1)
    got = {k: 0 for k in want}
    gotp = {q: 0 for q in partial}
    lines, tried = [], 0
    while time.time() < t_end - seconds * 0.35 and (any(got[k] < want[k] for k in want) or any(gotp[q] < 1 for q in partial)):
        tried += 1
        start = int(rng.choice([0, 3]))
        needp = [q for q in partial if gotp[q] < 1]
        quads = int(rng.choice(needp)) if needp and tried % 2 else 15
        ms = _tie_multiset(rng, int(valid_of(quads).sum()), start)
        if ms is None:
            continue
        counts, v1, v2 = ms
        recs = []
        for values in _layouts(rng, counts, quads, v1, v2, 8):
            rec = _rec(values, quads, start)
            if not recs and "tie_diff" not in classify(rec["model"], 0):
                break
            recs.append(rec)
        if not recs:
            continue
        if quads != 15:
            gotp[quads] += 1
            lines.append(_lit(f"part{quads}_tie_diff", recs[0]["values"], quads, start, "tie_diff"))
            continue
        pick = lambda rec: rec["model"]["pick"]
        wrong = {k: [rec for rec in recs if kernel_rule(rec, **kw) != pick(rec) and kernel_rule(rec) == pick(rec)]
                 for k, kw in (("shortcut_wide", dict(wide=True)), ("shortcut_diff", dict(ignore_diff=True)))}
        byp = {}
        for rec in recs:
            byp.setdefault(pick(rec), rec)
        fd = [rec for rec in recs if pick(rec) != rec["model"]["exact_pick"]]
        plain = [rec for rec in recs if pick(rec) == rec["model"]["exact_pick"]]
        for key in sorted(want, key=lambda k: got[k] - want[k]):
            if got[key] >= want[key]:
                continue
            if key.startswith("shortcut") and wrong[key]:
                lines.append(_lit(f"{key}_{got[key]}", wrong[key][0]["values"], 15, start, "tie_diff"))
            elif key == f"order{start}" and len(byp) > 1:
                a, b = list(byp.values())[:2]
                lines.append(_lit(f"order_s{start}_{got[key]}a", a["values"], 15, start, "order"))
                lines.append(_lit(f"order_s{start}_{got[key]}b", b["values"], 15, start, "order"))
            elif key == "float_decides" and fd:
                lines.append(_lit(f"float_decides_{got[key]}", fd[0]["values"], 15, start, "float_decides"))
            elif key == "tie_diff" and plain:
                lines.append(_lit(f"tie_diff_{got[key]}", plain[0]["values"], 15, start, "tie_diff"))
            else:
                continue
            got[key] += 1
            break
    print(f"# ties: {tried} multisets tried, found {got}, partial {gotp}")
    nnear, ntry = 0, 0
    while time.time() < t_end and nnear < 3:
        ntry += 1
        start = int(rng.choice([0, 3]))
        ms = _near_multiset(rng, start)
        if ms is None:
            continue
        counts, v1, v2 = ms
        for values in _layouts(rng, counts, 15, v1, v2, 0):
            if "near" in classify(tile_model(values, valid_of(15), start), 0):
                lines.append(_lit(f"near_{nnear}", values, 15, start, "near"))
                nnear += 1
            break
    print(f"# near: {ntry} triples tried, found {nnear}")
    print("\n".join(lines))


# ---- tiles by rule ---------------------------------------------------------------------------------------------------------------------------------
def _two_valued(lo: int, hi: int, n_hi: int) -> np.ndarray:
    """lo on the lattice, n_hi pixels of hi spread evenly over the other sixty"""
    rest = [hi if (i * n_hi) // 60 != ((i + 1) * n_hi) // 60 else lo for i in range(60)]
    return arrange(rest, 15, lo)


def _only(values, want: str) -> bool:
    """the tile's classes are exactly {want} for both start modes"""
    return all(classify(tile_model(values, valid_of(15), s)) == {want} for s in (0, 3))


REGIMES = {"hi224": (230, 250), "max255": (200, 255), "span_lt16": (100, 110), "span16_31": (100, 124), "span32": (100, 132), "span223": (10, 233),
           "zeros": (0, 90)}
SAME_SPANS = (0, 1, 7, 8, 100)


@functools.lru_cache(maxsize=None)
def made_tiles() -> dict:
    """Tiles that need no search, in the format of TILES (start None: the claim holds for both start modes).
      same_span<s>   tie_same and nothing else: two values s apart (one value for s = 0), the first minimum from 20 upwards that is such a tile
      zeros_tie      the same with zeros: {0, v}, the zeros' terms skipped
      zero_flat32    class zero: every pixel 32, which is its own table base (all minDiff 0); zero_black: every pixel 0 (all terms skipped)
      <regime>       REGIMES: random values from min to max, both present; no class claimed (flag None), the census must report min and max"""
    out = {}
    for s in SAME_SPANS:
        for mn in range(20, 200):
            v = _two_valued(mn, mn + s, 24)
            if _only(v, "tie_same"):
                out[f"same_span{s}"] = dict(quads=15, start=None, flag="tie_same", v=tuple(v.tolist()))
                break
    for hi in range(30, 200):
        v = _two_valued(0, hi, 24)
        if _only(v, "tie_same"):
            out["zeros_tie"] = dict(quads=15, start=None, flag="tie_same", v=tuple(v.tolist()))
            break
    for name, v in (("zero_flat32", 32), ("zero_black", 0)):
        out[name] = dict(quads=15, start=None, flag="zero", v=(v,) * 64)
    rng = np.random.default_rng(424242)
    for name, (mn, mx) in REGIMES.items():
        rest = rng.integers(mn, mx + 1, 60)
        rest[7], rest[40] = mx, mn
        out[name] = dict(quads=15, start=None, flag=None, v=tuple(arrange(rest, 15, mn).tolist()))
    return out


def tile(name: str) -> dict:
    return TILES[name] if name in TILES else made_tiles()[name]


def tile_c(name: str) -> int:
    """the value on the tile's lattice pixels: what a flat surround must hold"""
    t = tile(name)
    return int(next(t["v"][i] for i in LATTICE if valid_of(t["quads"])[i]))


# ---- the images ------------------------------------------------------------------------------------------------------------------------------------
class Image:
    """w x h pixels, three planes (plus alpha): random noise, which no gradient tile fits and whose tiles are coded whole, or one flat value,
    which the gradient tiles cover completely.  put() writes a tile into some planes; a cell the tile wants covered becomes flat in all
    planes, and so do the lattice pixels right of, below and diagonal to it, which are the other corners of its 4x4 gradient tile."""

    def __init__(self, w: int, h: int, seed: int, flat=None):
        self.w, self.h, self.flat = w, h, flat
        self.rng = np.random.default_rng(seed)
        self.p = self.rng.integers(0, 256, (3, h, w)) if flat is None else np.full((3, h, w), flat, np.int64)
        self.alpha, self.targets = None, []

    def cover(self, cy: int, cx: int, c: int):
        self.p[:, 4 * cy: 4 * cy + 4, 4 * cx: 4 * cx + 4] = c
        for dy, dx in ((0, 4), (4, 0), (4, 4)):
            assert 4 * cy + dy < self.h and 4 * cx + dx < self.w, "a covered cell on the image's edge"
            self.p[:, 4 * cy + dy, 4 * cx + dx] = c

    def noise_cell(self, cy: int, cx: int):
        """a cell no tile fits whose pixel (0, 0) keeps the surround's value: one more valid cell, and none of its neighbours is disturbed"""
        keep = self.p[:, 4 * cy, 4 * cx].copy()
        self.p[:, 4 * cy: 4 * cy + 4, 4 * cx: 4 * cx + 4] = self.rng.integers(0, 256, (3, 4, 4))
        self.p[:, 4 * cy, 4 * cx] = keep

    def put(self, name: str, ty: int, tx: int, planes=(0,), ctx: str = "", cover=None):
        t = tile(name)
        v, valid = np.asarray(t["v"], np.int64).reshape(8, 8), valid_of(t["quads"]).reshape(8, 8)
        c = tile_c(name)
        y, x = 8 * ty, 8 * tx
        pinned = self.flat is not None or t["quads"] != 15                  # the lattice pixels matter to the neighbours' gradient tiles
        assert self.flat is None or self.flat == c, (name, "needs a surround of", c)
        for p in range(3):
            blk = self.p[p, y: y + 8, x: x + 8]
            if p in planes:
                blk[valid] = v[valid]
            elif pinned:
                if self.flat is not None:
                    blk[valid] = self.rng.integers(0, 256, int(valid.sum()))
                for i in LATTICE:
                    if valid.ravel()[i]:
                        blk[i // 8, i % 8] = c
        for q in range(4):
            if not (t["quads"] >> q) & 1:
                self.cover(2 * ty + q // 2, 2 * tx + q % 2, c if cover is None else cover)
        for p in planes:
            self.targets.append({"name": name, "tile": (p, ty, tx), "flag": t["flag"], "start": t["start"], "quads": t["quads"], "ctx": ctx,
                                 "cover": cover})

    def planes(self) -> np.ndarray:
        out = self.p if self.alpha is None else np.concatenate([self.p, self.alpha[None]])
        assert out.min() >= 0 and out.max() <= 255
        out = np.ascontiguousarray(out, np.int32)
        out.setflags(write=False)
        return out


def whole_names() -> list:
    return [n for n in TILES if TILES[n]["quads"] == 15] + list(made_tiles())


PARTIAL = [(n, None) for n in TILES if TILES[n]["quads"] != 15] + [("part7_tie_diff", 250)]     # (tile, value of the covered cells: None = the tile's own)
SPREAD = ("part8_tie_diff", "part1_tie_diff", "part3_tie_diff", "part14_tie_diff", "order_s0_0a", "order_s0_0b", "shortcut_diff_1", "float_decides_2")
SPREAD_WHOLE_BLOCK = ("part8_tie_diff", "part14_tie_diff", "order_s0_0a")
TRI_SAME, TRI_MIXED = ("order_s3_2a", "order_s0_2b", "near_2"), ("order_s0_1b", "same_span100", None)   # tiles that go into all three planes; three planes in three classes


SERIAL = {3: ("order_s3_1b", "float_decides_4", "near_0", "order_s3_2b"), 0: ("order_s0_1a", "float_decides_1", "near_2", "order_s0_2b")}


def _fill(img: Image, names, slots, ctx: str):
    for i, (n, (ty, tx)) in enumerate(zip(names, slots)):
        img.put(n, ty, tx, (i % 3,), ctx)
    return len(names)


def _tri(img: Image, ty: int, tx: int):
    for i, n in enumerate(TRI_SAME):
        img.put(n, ty, tx + 2 + 2 * i, (0, 1, 2), "g: one tile in all three planes")
    for p, n in enumerate(TRI_MIXED):
        if n is not None:
            img.put(n, ty, tx, (p,), "g: three planes, three classes")
    img.mixed = (ty, tx)


def _build_full128x64():
    """every whole tile in a strip of whole tiles (a: fullTiles), up to eight ambiguous tiles per wave, side by side and one above the other
    (f); both sides a multiple of 64: the WHOLE instantiation's case"""
    img = Image(128, 64, 11)
    names = whole_names()
    n = _fill(img, names, [(i // 16, i % 16) for i in range(len(names))], "a: whole tiles; f: neighbours ambiguous too")
    _tri(img, n // 16 + 1, 2)
    for ty, names in ((4, SERIAL[3]), (6, SERIAL[0])):                      # f: four ambiguous tiles of ONE plane in ONE strip, for each start mode
        for name, (dy, tx) in zip(names, ((0, 8), (0, 9), (1, 8), (1, 15))):
            img.put(name, ty + dy, tx, (0,), "f: four ambiguous tiles of one plane in one strip")
    return img


def _build_full64x64():
    """one block of 64 x 64: the first literals again, and in strip row 2 an order pair next to a tile with one covered cell (a: a neighbour
    is partly covered, so the strip's stores take the general form)"""
    img = Image(64, 64, 12)
    names = [n for n in TILES if TILES[n]["quads"] == 15][:16]
    _fill(img, names, [(i // 8, i % 8) for i in range(16)], "a: whole tiles, one block")
    for n, tx in (("order_s0_1a", 1), ("order_s0_1b", 2), ("order_s3_1a", 5), ("near_0", 6)):
        img.put(n, 4, tx, (tx % 3,), "a: a neighbour of the strip is partly covered")
    img.cover(9, 7, 40)                                                     # tile (4, 3), its bottom-right cell
    img.partly = (4, 3)
    return img


def _build_noise72x40():
    """72 x 40: the ninth tile column and the fifth tile row are the last ones of a half macro-tile (w % 16 == 8, h % 16 == 8), the last strip
    row is ragged (d); the edge tiles are filled first"""
    img = Image(72, 40, 13)
    slots = [(ty, 8) for ty in range(5)] + [(4, tx) for tx in range(8)] + [(ty, tx) for ty in range(4) for tx in range(8)]
    names = [n for n in whole_names() if n.startswith(("order", "near", "shortcut", "float"))] + [n for n in whole_names() if n.startswith(("tie", "same", "zeros"))]
    _fill(img, names[: len(slots) - 2], slots, "d: last tile column / row first; general instantiation")
    return img


def _partial(w, h, seed, items, slots):
    img = Image(w, h, seed)
    for (n, cover), (ty, tx) in zip(items, slots):
        img.put(n, ty, tx, ((ty + tx) % 3,), "b: cells of the tile covered by 4x4 gradient tiles", cover)
    return img


def _build_spread(w, h, name, five: bool):
    """a flat image with ONE tile to code, in strip row 1: at most four valid cells, the kernel's `spread` path (c); five: noise cells bring the
    strip to five valid cells, the general path on the same tile"""
    img = Image(w, h, 15, flat=tile_c(name))
    img.put(name, 2, 3, (1,), "c: a strip of five valid cells" if five else "c: a strip of at most four valid cells")
    if five:
        for cy, cx in ((5, 10), (5, 12), (5, 14), (6, 11))[: 5 - bin(tile(name)["quads"]).count("1")]:
            img.noise_cell(cy, cx)
    img.strip = (16, 32, 0, 64)                                             # y0, y1, x0, x1 of the strip
    img.cells = 5 if five else bin(tile(name)["quads"]).count("1")
    return img


def _build_rgba64():
    """alpha: a kept box [16, 64) x [16, 64) (a shrunken bounding box) with the 16x16 tile at (32, 32) rejected (e); tiles right beside and
    above the rejected one.  The box starts at 16, so only its tiles up to x, y = 40 are coded (the reference's zero-size rule)."""
    img = Image(64, 64, 16)
    img.alpha = np.zeros((64, 64), np.int64)
    img.alpha[16:64, 16:64] = 255
    img.alpha[32:48, 32:48] = 0
    for n, ty, tx, p in (("order_s0_2a", 4, 3, 0), ("order_s0_2b", 3, 4, 1), ("order_s3_2a", 5, 3, 2), ("near_1", 2, 2, 0), ("shortcut_wide_0", 3, 5, 1)):
        img.put(n, ty, tx, (p,), "e: beside an alpha-rejected 16x16 tile, shrunken box")
    return img


PART_SLOTS_72 = [(ty, tx) for ty in (1, 3) for tx in (1, 3, 5, 7)]
BUILDERS = {
    "full128x64": _build_full128x64,
    "full64x64": _build_full64x64,
    "noise72x40": _build_noise72x40,
    "part72x40_a": lambda: _partial(72, 40, 21, PARTIAL[:7], PART_SLOTS_72),
    "part72x40_b": lambda: _partial(72, 40, 22, PARTIAL[7:], PART_SLOTS_72),
    "part128x64": lambda: _partial(128, 64, 23, PARTIAL, [(ty, tx) for ty in (1, 3, 5) for tx in range(1, 15, 2)]),
    "rgba64x64": _build_rgba64,
}
for _n in SPREAD:
    BUILDERS[f"spread72x40_{_n}"] = functools.partial(_build_spread, 72, 40, _n, False)
    BUILDERS[f"five72x40_{_n}"] = functools.partial(_build_spread, 72, 40, _n, True)
for _n in SPREAD_WHOLE_BLOCK:
    BUILDERS[f"spread64x64_{_n}"] = functools.partial(_build_spread, 64, 64, _n, False)
NAMES = tuple(BUILDERS)
WHOLE_NAMES = tuple(n for n in NAMES if "128x64" in n or "64x64" in n and not n.startswith("rgba"))   # RGB, both sides multiples of 64


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """{"name", "planes" int32 [3 or 4, h, w], "targets", "image" (the builder's record), "census": {mode3: census}}; computed once per process,
    never changed"""
    img = BUILDERS[name]()
    planes = img.planes()
    return {"name": name, "planes": planes, "targets": tuple(img.targets), "image": img, "census": {m3: census(planes, m3) for m3 in (False, True)}}


def claims(c: dict, mode3: bool):
    """the targets whose class is claimed under this start mode, with their census records: [(target, record or None)]"""
    start = 3 if mode3 else 0
    return [(t, c["census"][mode3]["tiles"].get(t["tile"])) for t in c["targets"] if t["start"] in (None, start)]


if __name__ == "__main__":
    import sys
    _search(float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)
