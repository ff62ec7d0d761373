"""TEST INFRASTRUCTURE ONLY.  Directed inputs for the gradient passes of the fused encode kernel, on top of tests/gradfit_cases.py: the deciding
pixel of a tile's last variant at EVERY column and row of a cell.

The kernel keeps the pixels of the gradient phase in stream layout (y2_rg / y2_bb in yaik_amd/csrc/yk_encode2.hip): channel 2 of the columns
(x, x + 1) of a cell shares a register, and the Round6P stream of channel 2 (stream 4) walks two pixels per operation with a row step of its
own per column.  A wrong row step or half select of column 1 or 2 cannot show in a tile whose deciding pixel sits in column 0 or 3, which is
where tests/gradfit_cases.py puts it.  Here, for every shape, every path of the kernel and the kinds "P4" (Round6P, channel 2: stream 4), "P3"
(Round6P, channels 0 | 1: stream 3) and "A" (a raw or Round6 variant), one tile per

    (first cell | last cell of the tile) x (column 0..3) x (row 0..3) x (sign) x (at rf: sole survivor | at rf + 1: the only failing pixel)

Pixel (0, 0) of a tile is its corner TL and cannot decide anything: UNREALISED lists those requests, and any other the generator could not
place (tests/test_gradfit_columns_cases.py asserts there is none).  One more image is 72 pixels wide: 8x8 tiles in the last tile column
inside the image (their right corners are clamped reads of column 71) with the deciding pixel in their last cell column."""
from __future__ import annotations

import functools

import numpy as np

from tests import gradfit_cases as gc
from tests.gradfit_cases import SHAPES, Canvas, census, paths_of

KINDS = ("P4", "P3", "A")
RF = 3
COLS, MAX_ROWS = 4, 8                        # strips per strip row and strip rows per image: the size of the ab* images of tests/gradfit_cases.py


def request_name(p, path, kind, cell, col, row, sign, expect) -> str:
    return f"{SHAPES[p][0]}x{SHAPES[p][1]}/{path}/{kind}/{cell}-cell/col{col}/row{row}/{'+' if sign > 0 else '-'}/{expect}"


def _decide(p, kind, cell, col, row, sign):
    """(variant, (channel, dx, dy, sign)) of a request: the variant and the channel walk through what the kind allows"""
    TX, TY = SHAPES[p]
    x0, y0 = (0, 0) if cell == "first" else (TX - 4, TY - 4)
    k = col + 2 * row + (1 if sign > 0 else 0) + (1 if cell == "last" else 0)
    if kind == "A":
        v, ch = k % 4, (col + row) % 3
    elif kind == "P3":
        v, ch = 4 + k % 2, (col + (row >> 1)) % 2
    else:
        v, ch = 4 + k % 2, 2
    return v, (ch, x0 + col, y0 + row, sign)


def all_requests():
    """[(name, pass, path, kind, variant, decide, expect)] and the names left out because the pixel is the corner TL"""
    reqs, corner = [], []
    for p in range(7):
        cells = ("first",) if SHAPES[p] == (4, 4) else ("first", "last")
        for path in paths_of(p):
            for kind in KINDS:
                for cell in cells:
                    for row in range(4):
                        for col in range(4):
                            for sign in (+1, -1):
                                for expect in ("sole", "reject"):
                                    name = request_name(p, path, kind, cell, col, row, sign, expect)
                                    v, dec = _decide(p, kind, cell, col, row, sign)
                                    if (dec[1], dec[2]) == (0, 0):
                                        corner.append(name)
                                    else:
                                        reqs.append((name, p, path, kind, v, dec, expect))
    return reqs, corner


def _pack(prefix, reqs, seed):
    """gradfit_cases._pack for requests that may fail: a request the generator cannot place leaves its macro-tile to the cells around it and
    goes to the second result.  One (pass, path) per strip; a strip row of 16x16 targets is followed by a dead one (their BL / BR corners),
    and every image ends with a dead strip row."""
    groups = {}
    for r in reqs:
        groups.setdefault((r[1], r[2]), []).append(r)
    strips = []
    for (p, path), rs in groups.items():
        cap = len(gc._slots(p, path, 0)[0])
        strips += [(p, path, rs[i: i + cap]) for i in range(0, len(rs), cap)]
    rows, cur = [], []
    for s in strips:
        if cur and (len(cur) == COLS or (SHAPES[cur[0][0]] == (16, 16)) != (SHAPES[s[0]] == (16, 16))):
            rows.append(cur); cur = []
        cur.append(s)
    if cur:
        rows.append(cur)
    images, failed, k = {}, [], 0
    while rows:
        take, used = [], 0
        while rows and used + 2 <= MAX_ROWS:
            used += 2 if SHAPES[rows[0][0][0]] == (16, 16) else 1
            take.append(rows.pop(0))
        nrows = used + (0 if SHAPES[take[-1][0][0]] == (16, 16) else 1)
        cv = Canvas(64 * COLS, 16 * nrows, RF, seed + k)
        r = 0
        for row in take:
            for col, (p, path, rs) in enumerate(row):
                mts, around, others = gc._slots(p, path, r)
                for m in range(4):
                    cv.fill(4 * r, 16 * col + 4 * m, 4, 4, around if m in mts else others[m])
                for m, (name, _, _, kind, v, dec, expect) in zip(mts, rs):
                    out = cv.place(p, 4 * r, 16 * col + 4 * m, gc._sole(v, dec, expect == "reject")(SHAPES[p], RF),
                                   group="K", request=name, kind=kind, variant=v, decide=dec, expect=expect, path=path)
                    if out is None:
                        failed.append(name)
            r += 2 if SHAPES[row[0][0]] == (16, 16) else 1
        images[f"{prefix}_{k}"] = cv
        k += 1
    return images, failed


W72 = (72, 72)
W72_PIXELS = ((5, 2, +1), (6, 1, -1))        # (dx, dy, sign) in the last cell column of an 8x8 tile: columns 1 and 2 of that cell


def _build_w72():
    """72 x 72: one 8x8 target per strip row at x = 64, the last tile column inside the image.  Its TR corner is the clamped read of column 71,
    that is its own pixel (7, 0); BL and BR are pixel (0, 0) and row 0 of the plugs below it.  Stream 4 decides at the pixels of W72_PIXELS."""
    w, h = W72
    cv = Canvas(w, h, RF, 8100)
    todo = [(dx, dy, sign, expect) for dx, dy, sign in W72_PIXELS for expect in ("sole", "reject")]
    assert len(todo) * 16 + 8 == h
    failed = []
    for i, (dx, dy, sign, expect) in enumerate(todo):
        cy, cx, want = 4 * i, 16, 4 + i % 2
        dec = (2, dx, dy, sign)
        name = f"w72/8x8/P4/col{dx % 4}/row{dy}/{'+' if sign > 0 else '-'}/{expect}"
        for _ in range(2000):
            tl = cv.rng.integers(60, 190, 3)
            corners = np.array([tl] + [np.clip(tl + cv.rng.integers(-8, 9, 3), 0, 255) for _ in range(3)], np.int64)
            cur = gc._synth(cv.rng, corners, 8, 8, RF, want, dec, expect == "reject")
            if cur is None:
                continue
            cur[:, 0, 7] = corners[1]                                      # the clamped TR is a pixel of the tile
            ok, first, nf = gc._variants_many(cur[None], corners[None], 8, 8, RF)
            alive = set(np.nonzero(ok[0])[0].tolist())
            if gc._tile_dead(cur, RF):
                continue
            if expect == "reject" and (alive or nf[0, want] != 1 or first[0, want] != (dy * 8 + dx) * 3 + 2):
                continue
            if expect == "sole" and alive != {want}:
                continue
            break
        else:
            failed.append(name)
            continue
        cv.kind[cy: cy + 2, cx: cx + 2] = "t"
        cv.kind[cy + 2, cx: cx + 2] = "p"
        cv.lat[(cy + 2, cx)], cv.lat[(cy + 2, cx + 1)] = corners[2], corners[3]
        cv.tiles.append((4 * cy, 4 * cx, cur))
        cv.targets.append(dict(group="W", request=name, p=3, cy=cy, cx=cx, kind="P4", variant=want, decide=dec, expect=expect, path="compact"))
    return {"kw72": cv}, failed


@functools.lru_cache(maxsize=None)
def _built():
    reqs, corner = all_requests()
    images, failed = {}, []
    for p in range(7):
        im, f = _pack(f"k{SHAPES[p][0]}x{SHAPES[p][1]}", [r for r in reqs if r[1] == p], 9000 + 100 * p)
        images.update(im); failed += f
    im, f = _build_w72()
    images.update(im); failed += f
    return images, tuple(corner), tuple(failed)


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """like gradfit_cases.case: {"name", "planes" int32 [3, h, w], "rf", "targets", "census"}; computed once per process, never changed.
    "<name>@rot1" / "@rot2": the same image with its channels rotated, a frame of the same shape for the batches (no targets claimed)."""
    base, _, rot = name.partition("@rot")
    cv = _built()[0][base]
    planes = cv.render() if not rot else np.ascontiguousarray(np.roll(case(base)["planes"], int(rot), axis=0))
    planes.setflags(write=False)
    return {"name": name, "planes": planes, "rf": cv.rf, "targets": () if rot else tuple(cv.targets), "census": census(planes, cv.rf)}


def _batches():
    """every image in one batch of three different frames of its shape; a shape with fewer than three images is filled up with channel-rotated
    copies of its first, a count that is no multiple of three ends with an overlapping triple"""
    groups = {}
    for n in ALL_NAMES:
        cv = _built()[0][n]
        groups.setdefault((cv.w, cv.h), []).append(n)
    out = []
    for pool in groups.values():
        pool = pool + [f"{pool[0]}@rot{r}" for r in (1, 2)][: max(0, 3 - len(pool))]
        out += [tuple(pool[i: i + 3]) for i in range(0, len(pool) - 2, 3)] + ([tuple(pool[-3:])] if len(pool) % 3 else [])
    return tuple(out)


ALL_NAMES = tuple(_built()[0])
CORNER_REQUESTS = _built()[1]                # left out by construction: pixel (0, 0) of the tile
UNREALISED = CORNER_REQUESTS + _built()[2]   # every request no image holds, by name
BATCHES = _batches()
