// The clip of yk_window_px.h with a horizontal mirror on top (yk_decode_output_norm_device and its kin).  No HIP in here: yk_decode.hip
// includes it inside the normalising de-tile kernel and for the host checks, yaik_amd/host/window_mirror_tool.cpp runs it against a brute-force
// enumeration for the `not gpu` tests -- a wrong value would be an out-of-bounds store on the device.
#pragma once
#include "yk_window_px.h"

// The 8-pixel segment of cover tile column j against a window that starts d pixels into the cover and is ww pixels long (yk_wpx_clip), written
// plain or mirrored: columns src0 .. src0 + n - 1 of the segment are kept, and they fill destination columns dst .. dst + n - 1.
//   mirror == 0: segment column src0 + i goes to dst + i            (yk_wpx_clip itself)
//   mirror != 0: segment column src0 + i goes to dst + n - 1 - i    (window column x lands at ww - 1 - x)
// dst is the leftmost destination column written either way, so [dst, dst + n) is what a store may touch: 0 <= dst, dst + n <= ww.
struct YkPxMirrorClip { int src0, n, dst; };
YK_WPX_FN YkPxMirrorClip yk_wpx_clip_mirror(int j, int d, int ww, int mirror) {
    const YkPxClip k = yk_wpx_clip(j, d, ww);
    if (k.n == 0) return YkPxMirrorClip{ 0, 0, 0 };
    return YkPxMirrorClip{ k.src0, k.n, mirror ? ww - k.dst - k.n : k.dst };
}
// The kernel reverses a mirrored segment in registers first (column c becomes column 7 - c) and then stores kept columns in rising order: the kept
// columns of the reversed segment start here.
YK_WPX_FN int yk_wpx_mirror_src0(const YkPxMirrorClip k, int mirror) { return mirror ? 8 - k.src0 - k.n : k.src0; }

// the rule of the normalisation parameters: finite, and 0 or of magnitude in [2^-100, 2^100] (then no fp32 intermediate of v * scale + bias, v = 0..255,
// is subnormal or overflows, whatever the denormal mode)
YK_WPX_FN bool yk_norm_param_ok(float v) {
    const float a = v < 0 ? -v : v;
    if (!(a == a)) return false;                                 // NaN
    if (a == 0.0f) return true;
    return a >= 0x1p-100f && a <= 0x1p100f;                      // infinity fails the upper bound
}
