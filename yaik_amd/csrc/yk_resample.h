// Rectangles resampled to one output size (yk_decode_set_batch_rects, yk_decode_output_resampled_*): the whole arithmetic of the
// contract, in integers.  No HIP in here: yk_decode.hip includes it inside the resample kernel and for the host checks, yaik_decode.cpp for the
// checks that come before a slot is taken, and yaik_amd/host/resample_tool.cpp runs it against a brute-force 64-bit and rational form for the
// `not gpu` tests -- a wrong tap would be an out-of-bounds load on the device.  One axis at a time: x with (sw, ow), y with (sh, oh).
//
//     step   = floor(n_src * 65536 / n_out)                    16.16 source pixels per output pixel
//     off    = (step >> 1) - 32768                             half-pixel centres: (i + 0.5) * n_src / n_out - 0.5
//     pos(i) = clamp(off + i * step, 0, (n_src - 1) << 16)     i = 0 .. n_out - 1
//     i0 = pos >> 16,  f = (pos >> 8) & 255,  i1 = min(i0 + 1, n_src - 1)
//     v  = ((a (256 - fx) + b fx) (256 - fy) + (c (256 - fx) + d fx) fy + 32768) >> 16
//
// With 1 <= n_src, n_out <= YK_RS_MAX every value fits a signed 32-bit integer: step <= 2^30, off + i * step < 2^30 + 2^29, the blend < 2^25.
#pragma once
#include "yk_window_px.h"

#define YK_RS_MAX 16384                                     // the largest source rectangle side and the largest output side
#define YK_RS_WORDS 9                                       // per frame in HBM: x0, y0, sw - 1, sh - 1, stepX, offX, stepY, offY, mirror

struct YkRsAxis { int step, off; };
struct YkRsTap { int i0, i1, f; };

// the host computes step in 64 bits (n_src << 16 is 2^30 at most, so 32 bits would do: the tool checks that too)
YK_WPX_FN YkRsAxis yk_rs_axis(int n_src, int n_out) {
    const int step = (int)(((long long)n_src << 16) / n_out);
    return YkRsAxis{ step, (step >> 1) - 32768 };
}
// the taps of output index i on an axis of n_src source pixels: both inside 0 .. n_src - 1
YK_WPX_FN YkRsTap yk_rs_tap(const YkRsAxis ax, int i, int n_src) {
    const int last = n_src - 1;
    int pos = ax.off + i * ax.step;
    pos = pos < 0 ? 0 : pos;
    pos = pos > (last << 16) ? (last << 16) : pos;
    const int i0 = pos >> 16;
    return YkRsTap{ i0, i0 < last ? i0 + 1 : last, (pos >> 8) & 255 };
}
// a b / c d: the bytes at (i0, j0), (i1, j0), (i0, j1), (i1, j1)
YK_WPX_FN int yk_rs_blend(int a, int b, int c, int d, int fx, int fy) {
    const int top = a * (256 - fx) + b * fx, bot = c * (256 - fx) + d * fx;
    return (top * (256 - fy) + bot * fy + 32768) >> 16;
}

// the rule: a source rectangle of sw x sh pixels at (x0, y0) inside a w x h image, no alignment, and an output of ow x oh
YK_WPX_FN bool yk_rs_size_ok(int ow, int oh) { return ow >= 1 && oh >= 1 && ow <= YK_RS_MAX && oh <= YK_RS_MAX; }
YK_WPX_FN bool yk_rs_src_ok(int x0, int y0, int sw, int sh, int w, int h) { return yk_wpx_window_ok(x0, y0, sw, sh, w, h) && sw <= YK_RS_MAX && sh <= YK_RS_MAX; }
YK_WPX_FN bool yk_rs_rect_ok(int x0, int y0, int sw, int sh, int w, int h, int ow, int oh) { return yk_rs_src_ok(x0, y0, sw, sh, w, h) && yk_rs_size_ok(ow, oh); }

// The cover of frame f's rectangle: the smallest 8-aligned rectangle that contains it (yk_wpx_cover per axis), with no size shared by the batch.
// It is all the chunk calls decode, because the taps never leave the rectangle.
struct YkRsCover { int x0, y0, x1, y1; };
YK_WPX_FN YkRsCover yk_rs_cover(int x0, int y0, int sw, int sh) {
    const YkPxCover cx = yk_wpx_cover(x0, sw), cy = yk_wpx_cover(y0, sh);
    return YkRsCover{ cx.c0, cy.c0, cx.c0 + cx.cw, cy.c0 + cy.cw };
}

// the nine words of a frame
YK_WPX_FN void yk_rs_words(int x0, int y0, int sw, int sh, int ow, int oh, int mirror, int* t) {
    const YkRsAxis ax = yk_rs_axis(sw, ow), ay = yk_rs_axis(sh, oh);
    t[0] = x0; t[1] = y0; t[2] = sw - 1; t[3] = sh - 1; t[4] = ax.step; t[5] = ax.off; t[6] = ay.step; t[7] = ay.off; t[8] = mirror ? 1 : 0;
}
