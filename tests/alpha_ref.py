"""From-scratch numpy restatement of the 'ALPM' alpha value coder (test infrastructure).

encode(): EncoderContext::ProcessAlpha(force8Bit) (encoder/EncoderContext.cpp:1429-1682, make1BitStream :317-355) on a u8 alpha
plane, the MipPrefilter bounds and its per-pixel mask.  decode(): the four unpackers of decoder/YAIK_Alpha.cpp on the decompressed
payload.  Both follow the reference's loops as they execute; the readings of its undefined spots are the ones DESIGN.md lists.
"""
from __future__ import annotations

import numpy as np

IS_1_BIT_USEMIPMAPMASK = 0
IS_1_BIT_FULL = 1
IS_6_BIT_USEMIPMAPMASK = 2
IS_6_BIT_USEMIPMAPMASK_INVERSE = 3
IS_6_BIT_FULL = 4
IS_6_BIT_FULL_INVERSE = 5
IS_8_BIT_FULL = 6


def pack6(values: np.ndarray) -> np.ndarray:
    """Four 6-bit values into three bytes, LSB first; a partial last group keeps only the bytes it touched (:1528-1551)."""
    v = np.asarray(values, dtype=np.uint32).ravel()
    n = v.size
    pad = np.zeros((n + 3) // 4 * 4, dtype=np.uint32)
    pad[:n] = v
    a, b, c, d = pad[0::4], pad[1::4], pad[2::4], pad[3::4]
    out = np.stack([(a | (b << 6)) & 255, ((b >> 2) | (c << 4)) & 255, ((c >> 4) | (d << 2)) & 255], axis=1).astype(np.uint8).ravel()
    return out[: (n // 4) * 3 + (0, 1, 2, 3)[n % 4]]


def unpack6(stream: np.ndarray, count: int) -> np.ndarray:
    s = np.zeros((count + 3) // 4 * 3, dtype=np.uint32)
    src = np.asarray(stream, dtype=np.uint8)[: s.size]
    s[: src.size] = src
    b0, b1, b2 = s[0::3], s[1::3], s[2::3]
    v = np.stack([b0 & 63, (b0 >> 6) | ((b1 & 15) << 2), (b1 >> 4) | ((b2 & 3) << 4), b2 >> 2], axis=1).ravel()
    return v[:count]


def expand6(x: np.ndarray, inverse: bool) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint32)
    if inverse:
        x = 63 - x
    return ((x << 2) | (x >> 4)).astype(np.uint8)


def encode(alpha: np.ndarray, bounds, mask: np.ndarray | None, force8bit: bool = True):
    """None when ProcessAlpha writes no chunk, else dict(mode, bbox=(x, y, w, h), payload=u8 array).
    bounds = (boundX0, boundY0, boundX1, boundY1); mask = the per-pixel mipmapMask (non-zero = selected), needed for force8bit=False."""
    a = np.asarray(alpha, dtype=np.int64)
    x0, y0, x1, y1 = (int(v) for v in bounds)
    sub = a[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)]
    ys, xs = np.nonzero(sub >> 2)
    if ys.size == 0:
        return None                                    # empty box: the class loop never runs, isAll0 and isAll1 stay true
    bL, bR = x0 + int(xs.min()), x0 + int(xs.max()) + 1
    bT, bB = y0 + int(ys.min()), y0 + int(ys.max()) + 1
    bL, bR = (bL >> 2) << 2, ((bR + 3) >> 2) << 2
    box = a[bT:bB, bL:bR]
    analog = bool(np.any((box > 0) & (box < 255)))
    all1 = bool(np.all(box == 255))
    all0 = bool(np.all(box == 0))
    if not analog and not all0 and not all1:          # binary: the box re-aligned to 8, one bit per sample, no mask
        bL, bR = (bL >> 3) << 3, ((bR + 7) >> 3) << 3
        bits = (a[bT:bB, bL:bR] & 1).astype(np.uint8).ravel()
        return dict(mode=IS_1_BIT_FULL, bbox=(bL, bT, bR - bL, bB - bT), payload=np.packbits(bits, bitorder="little"))
    if not analog:
        return None
    if force8bit:
        return dict(mode=IS_8_BIT_FULL, bbox=(bL, bT, bR - bL, bB - bT), payload=box.astype(np.uint8).ravel())
    sel = box[np.asarray(mask)[bT:bB, bL:bR] != 0]    # row-major, mask-selected samples only
    return dict(mode=IS_6_BIT_USEMIPMAPMASK_INVERSE, bbox=(bL, bT, bR - bL, bB - bT), payload=pack6(63 - (sel >> 2)))


def decode(mode: int, bbox, payload: np.ndarray, w: int, h: int, mask: np.ndarray | None = None, mask_bbox=None,
           reference_1bit: bool = True) -> np.ndarray:
    """The w x h plane an unpacker leaves (bytes it never writes are 0).  mask = the decoder's mipMapMask bytes, mask_bbox its box in
    pixels.  reference_1bit: the 1-bit row loop as the reference runs it (`while (--cnt)`: w/8 - 1 bytes per row, rows drifting 8
    pixels left); False = w/8 bytes per row, the layout make1BitStream writes."""
    bx, by, bw, bh = (int(v) for v in bbox)
    p = np.asarray(payload, dtype=np.uint8)
    out = np.zeros(w * h, dtype=np.uint8)
    if mode == IS_8_BIT_FULL:
        out.reshape(h, w)[by:by + bh, bx:bx + bw] = p[: bw * bh].reshape(bh, bw)
    elif mode in (IS_6_BIT_FULL, IS_6_BIT_FULL_INVERSE):
        v = unpack6(p, bw * bh).reshape(bh, bw)
        out.reshape(h, w)[by:by + bh, bx:bx + bw] = expand6(v, mode == IS_6_BIT_FULL_INVERSE)
    elif mode == IS_1_BIT_FULL:
        blk = bw >> 3
        per = blk - 1 if reference_1bit else blk
        bits = np.unpackbits(p[: per * bh], bitorder="little").reshape(bh, per * 8).astype(np.uint8) * 255
        if reference_1bit:
            start = by * w + bx
            for r in range(bh):
                out[start + r * (w - 8): start + r * (w - 8) + per * 8] = bits[r]
        else:
            out.reshape(h, w)[by:by + bh, bx:bx + bw] = bits
    elif mode in (IS_6_BIT_USEMIPMAPMASK, IS_6_BIT_USEMIPMAPMASK_INVERSE):
        m = np.asarray(mask, dtype=np.uint8)
        stride = int(mask_bbox[2])
        base = ((bx - int(mask_bbox[0])) + stride * (by - int(mask_bbox[1]))) & 0xFFFFFFFF
        r, c = np.mgrid[0:bh, 0:bw]
        pos = (base + stride * r.astype(np.int64) + c) & 0xFFFFFFFF
        inside = (pos >> 3) < m.size
        sel = np.zeros((bh, bw), dtype=bool)
        sel[inside] = ((m[(pos[inside] >> 3)] >> (pos[inside] & 7)) & 1) != 0
        n = int(sel.sum())
        vals = expand6(unpack6(p, n), mode == IS_6_BIT_USEMIPMAPMASK_INVERSE)
        box = np.zeros((bh, bw), dtype=np.uint8)
        box[sel] = vals
        out.reshape(h, w)[by:by + bh, bx:bx + bw] = box
    else:
        raise ValueError(f"alpha mode {mode} has no unpacker")
    return out.reshape(h, w)


def swizzled_mask(tile_bits: np.ndarray, tbw: int, tbh: int) -> np.ndarray:
    """Decompress1BitTiled (decoder/YAIK_Mipmap.cpp:112-137): 1 bit per 16x16 tile -> the decoder's swizzled mask bytes."""
    out = np.zeros(tbw * tbh * 32, dtype=np.uint8)
    bits = np.unpackbits(np.asarray(tile_bits, dtype=np.uint8), bitorder="little")
    o = out.reshape(tbh, 2, tbw, 16)                   # per tile row: tileA half (2 u64 per tile), then tileB half
    for ty in range(tbh):
        for tx in range(tbw):
            if bits[ty * tbw + tx]:
                o[ty, :, tx, :] = 255
    return out
