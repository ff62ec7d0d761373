// Windows at any pixel offset and size (yk_decode_set_window_px and its kin): the rule, the 8-aligned cover the upstream stages decode,
// and the clip of one 8-pixel segment of the cover against the window.  No HIP in here: yk_decode.hip includes it for the checks and inside the
// clipping de-tile kernels, yaik_amd/host/window_px_tool.cpp runs the same functions exhaustively for the `not gpu` tests -- a wrong value would be
// an out-of-bounds store on the device, so the logic is tested on the CPU before it feeds a launch.  One axis at a time: every function serves x
// with (x0, ww, w) and y with (y0, wh, h).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YK_WPX_FN __host__ __device__ inline
#else
#define YK_WPX_FN inline
#endif

// the rule on one axis: a window of ww >= 1 pixels at x0 >= 0 inside an image of w pixels, no alignment (overflow-safe: x0 > w - ww, never x0 + ww)
YK_WPX_FN bool yk_wpx_axis_ok(int x0, int ww, int w) { return x0 >= 0 && ww >= 1 && ww <= w && x0 <= w - ww; }
YK_WPX_FN bool yk_wpx_window_ok(int x0, int y0, int ww, int wh, int w, int h) { return yk_wpx_axis_ok(x0, ww, w) && yk_wpx_axis_ok(y0, wh, h); }
YK_WPX_FN bool yk_wpx_windows_ok(int n, const int* xy, int ww, int wh, int w, int h) {
    if (n < 1 || !xy) return false;
    for (int k = 0; k < n; k++)
        if (!yk_wpx_window_ok(xy[2 * k], xy[2 * k + 1], ww, wh, w, h)) return false;
    return true;
}
// a window the aligned calls take as it is
YK_WPX_FN bool yk_wpx_aligned(int x0, int y0, int ww, int wh) { return ((x0 | y0 | ww | wh) & 7) == 0; }

struct YkPxCover { int c0, cw; };                           // one axis of a cover: origin and size, both multiples of 8

// The cover of one window: the smallest 8-aligned interval that contains [x0, x0 + ww).  It lies inside the image because w is a multiple of 8.
YK_WPX_FN YkPxCover yk_wpx_cover(int x0, int ww) {
    const int c0 = x0 & ~7;
    return YkPxCover{ c0, ((x0 + ww + 7) & ~7) - c0 };
}
// The shared cover of a batch or a multi-window call, whose kernels take one tile count for every window: the size depends on (ww, w) only,
// cw = min(w, 8 ceil((ww + 7) / 8)), wide enough for every residue of x0; the origin is x0 & ~7 pulled back inside the image at the far edge.
// c0 <= x0, x0 + ww <= c0 + cw <= w, cw - ww < 16; the offset x0 - c0 may exceed 7 where the cover was pulled back.
YK_WPX_FN int yk_wpx_shared_size(int ww, int w) {
    const int cw = ((ww + 7 + 7) >> 3) << 3;
    return cw < w ? cw : w;
}
YK_WPX_FN YkPxCover yk_wpx_shared_cover(int x0, int ww, int w) {
    const int cw = yk_wpx_shared_size(ww, w), a0 = x0 & ~7;
    return YkPxCover{ a0 < w - cw ? a0 : w - cw, cw };
}

// The clip of the 8-pixel segment of cover tile column j (cover pixels 8j .. 8j + 7) against a window that starts d = x0 - c0 pixels into the
// cover and is ww pixels long: columns src0 .. src0 + n - 1 of the segment go to window columns dst .. dst + n - 1.  n is 0..8; d is any
// value >= 0.  With (jy, dy, wh) the same function clips the rows of a tile.
struct YkPxClip { int src0, n, dst; };
YK_WPX_FN YkPxClip yk_wpx_clip(int j, int d, int ww) {
    const int s = 8 * j;
    const int lo = s > d ? s : d, hi = s + 8 < d + ww ? s + 8 : d + ww;
    if (hi <= lo) return YkPxClip{ 0, 0, 0 };
    return YkPxClip{ lo - s, hi - lo, lo - d };
}
