// Which 64x64 blocks of a prepared image a set of windows still needs rendered (yk_decode_render_windows_device).  No HIP in here:
// yk_decode.hip includes it for the handle's bookkeeping, yaik_amd/host/window_blocks_tool.cpp for the `not gpu` tests -- a wrong block id would
// be an out-of-bounds access on the device, so the logic is tested on the CPU before it feeds a launch.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>

// One bit per 64x64 block of the image, block (bx, by) = bit by * nbx + bx: `done` = rendered since the image was prepared.
struct YkWindowBlocks {
    int w = 0, h = 0, nbx = 0, nby = 0, rendered = 0;
    std::vector<uint64_t> done, fresh;                      // fresh: scratch of yk_wb_take, all zero between calls
};

inline void yk_wb_reset(YkWindowBlocks& B, int w, int h) {
    B.w = w; B.h = h; B.nbx = (w + 63) / 64; B.nby = (h + 63) / 64; B.rendered = 0;
    const size_t words = ((size_t)B.nbx * B.nby + 63) / 64;
    B.done.assign(words, 0); B.fresh.assign(words, 0);
}
inline int yk_wb_total(const YkWindowBlocks& B) { return B.nbx * B.nby; }

// the rule of yk_decode_set_window for n windows of one size: multiples of 8, at least 8 x 8, inside the image
inline bool yk_wb_windows_ok(const YkWindowBlocks& B, int n, const int* xy, int ww, int wh) {
    if (n < 1 || !xy || ((ww | wh) & 7) || ww < 8 || wh < 8 || ww > B.w || wh > B.h) return false;
    for (int k = 0; k < n; k++) {
        const int x0 = xy[2 * k], y0 = xy[2 * k + 1];
        if (((x0 | y0) & 7) || x0 < 0 || y0 < 0 || x0 > B.w - ww || y0 > B.h - wh) return false;
    }
    return true;
}

// The blocks the union of the windows touches that are not rendered yet: ascending, each once however many windows touch it; they count as
// rendered from here on.  The windows have passed yk_wb_windows_ok.
inline void yk_wb_take(YkWindowBlocks& B, int n, const int* xy, int ww, int wh, std::vector<uint32_t>& list) {
    list.clear();
    size_t lo = B.fresh.size(), hi = 0;                     // words of `fresh` that got a bit
    for (int k = 0; k < n; k++) {
        const int bx0 = xy[2 * k] >> 6, by0 = xy[2 * k + 1] >> 6, bx1 = (xy[2 * k] + ww - 1) >> 6, by1 = (xy[2 * k + 1] + wh - 1) >> 6;
        for (int by = by0; by <= by1; by++)
            for (int bx = bx0; bx <= bx1; bx++) {
                const size_t b = (size_t)by * B.nbx + bx, wd = b >> 6;
                const uint64_t bit = (uint64_t)1 << (b & 63);
                if (B.done[wd] & bit) continue;
                B.fresh[wd] |= bit;
                if (wd < lo) lo = wd;
                if (wd > hi) hi = wd;
            }
    }
    for (size_t wd = lo; wd <= hi && wd < B.fresh.size(); wd++) {
        uint64_t m = B.fresh[wd];
        if (!m) continue;
        B.done[wd] |= m; B.fresh[wd] = 0;
        while (m) { list.push_back((uint32_t)(wd * 64 + (size_t)__builtin_ctzll(m))); m &= m - 1; }
    }
    B.rendered += (int)list.size();
}
