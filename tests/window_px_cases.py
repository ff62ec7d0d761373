"""Shared pieces of the pixel-window decode tests (yk_decode_set_window_px and its kin): the windows of every image of
tests/window_cases.py, at any pixel offset and size, and the origin sets of the multi-window and batch calls.  The expected pixels are always
ref.rgb[y0:y0 + wh, x0:x0 + ww] of the oracle's whole decode (WC.reference, BW.batch_references).

Everything upstream of the de-tile runs on the window's 8-aligned cover and is pinned by the aligned tests; the new ground is the clip, so the
windows aim at it: single pixels, pixels across a tile corner, every residue of origin and size modulo 8, the far edges, and covers that equal
the windows the aligned tests already condition (WC.SCAN_BLOCK_WINDOW, WC.STRADDLE)."""
from tests import window_cases as WC

# the window whose cover is WC.SCAN_BLOCK_WINDOW = (192, 112, 192, 40), and per mixed image the one whose cover is WC.STRADDLE
SCAN_BLOCK_PX = (195, 117, 186, 30)
STRADDLE_PX = {(136, 264): (57, 59, 21, 11), (520, 264): (251, 185, 11, 14)}
RESIDUES = [(8 + d, 16 + (5 * d) % 8, 9 + d, 23 - d) for d in range(8)]
# the shared sizes of the multi-window and batch calls; (0, 0) stands for the whole image
SHARED_SIZES = [(13, 11), (100, 37), (1, 1), (0, 0)]


def cover(win) -> tuple:
    """the smallest 8-aligned rectangle that contains the window"""
    x0, y0, ww, wh = win
    cx, cy = x0 & ~7, y0 & ~7
    return cx, cy, ((x0 + ww + 7) & ~7) - cx, ((y0 + wh + 7) & ~7) - cy


def shared_cover(win, w: int, h: int) -> tuple:
    """the cover of one size for every origin (multi-window and batch calls): min(w, 8 ceil((ww + 7) / 8)) wide at x0 & ~7, pulled back inside the image"""
    x0, y0, ww, wh = win
    cw, ch = min(w, (ww + 14) // 8 * 8), min(h, (wh + 14) // 8 * 8)
    return min(x0 & ~7, w - cw), min(y0 & ~7, h - ch), cw, ch


def inside(win, w: int, h: int) -> bool:
    x0, y0, ww, wh = win
    return x0 >= 0 and y0 >= 0 and ww >= 1 and wh >= 1 and x0 + ww <= w and y0 + wh <= h


def windows(w: int, h: int) -> list:
    """the pixel windows (x0, y0, ww, wh) of a w x h image, without repeats; an 8 x 8 image takes those that fit"""
    out = [(0, 0, w, h), (1, 1, w - 2, h - 2),                          # the whole image, and with a 1-pixel border removed
           (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (3, 5, 1, 1),            # single pixels
           (7, 7, 2, 2),                                                # two pixels across a tile corner
           (9, 10, 5, 4),                                               # inside one tile
           (w - 3, 0, 1, h), (0, h - 2, w, 1),                          # one column, one row
           (w - 13, h - 11, 13, 11),                                    # unaligned at the right and bottom edge
           (61, 59, 7, 9)]                                              # across the corner of four 64-blocks
    out += RESIDUES
    if (w, h) == (520, 264):
        out.append(SCAN_BLOCK_PX)
    if (w, h) in STRADDLE_PX:
        out.append(STRADDLE_PX[(w, h)])
    seen, uniq = set(), []
    for win in out:
        if inside(win, w, h) and win not in seen:
            seen.add(win)
            uniq.append(win)
    return uniq


def all_case_windows() -> list:
    return [(w, h, kind, win) for w, h, kind in WC.CASES for win in windows(w, h)]


def origin_sets(w: int, h: int, n: int | None = None) -> list:
    """[((ww, wh), origins)] for the multi-window and batch calls of a w x h image: per shared size that fits, origins that include (0, 0), the
    far corner (w - ww, h - wh) -- where the shared cover is pulled back and the offset into it exceeds 7 -- two that overlap and a mix of
    residues.  n: that many origins (a batch of n frames), pairwise different unless the size leaves one origin only."""
    sets = []
    for ww, wh in SHARED_SIZES:
        if (ww, wh) == (0, 0):
            ww, wh = w, h
        if ww > w or wh > h:
            continue
        mx, my = w - ww, h - wh
        cand = [(0, 0), (mx, my), (min(3, mx), min(5, my)), (min(9, mx), min(10, my)), (mx // 2 | 1 if mx > 1 else 0, my // 3), (min(6, mx), my), (mx, min(7, my)),
                (min(20, mx), min(17, my))]
        origins = []
        for o in cand:
            if o not in origins:
                origins.append(o)
        if n is not None:
            origins = (origins * n)[:n] if len(origins) < n else origins[:n]
        sets.append(((ww, wh), origins))
    return sets


def touched_blocks(w: int, h: int, origins, ww: int, wh: int) -> int:
    """how many 64x64 blocks of the image the pixel rectangles touch"""
    blocks = set()
    for x0, y0 in origins:
        for by in range(y0 // 64, (y0 + wh - 1) // 64 + 1):
            for bx in range(x0 // 64, (x0 + ww - 1) // 64 + 1):
                blocks.add((bx, by))
    return len(blocks)
