// CPU-only: the cover and clip arithmetic of the pixel-window calls (yaik_amd/csrc/yk_window_px.h, no HIP linked), for the `not gpu` tests.
//   window_px_tool check <w>          every window (x0, ww) the rule allows on an axis of w pixels, and every one just outside it:
//                                     prints "ok <windows checked>", or the first failure and exit status 1
//   window_px_tool show <w> <x0> <ww> one window:  "<c0> <cw> <s0> <sw> :" and then "<j>,<src0>,<n>,<dst>" for every tile column j of the shared
//                                     cover (c0, cw the single cover, s0, sw the shared one);  a window outside the rule:  "bad", exit status 3
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../csrc/yk_window_px.h"

#define FAIL(...) do { printf("FAIL w=%d x0=%d ww=%d: ", w, x0, ww); printf(__VA_ARGS__); printf("\n"); return false; } while (0)

// the union over the cover's tile columns of what the clip keeps is [0, ww), each column once, from source columns inside the cover
static bool check_clip(int w, int x0, int ww, const YkPxCover cv) {
    std::vector<int> seen((size_t)ww, 0);
    const int d = x0 - cv.c0;
    for (int j = 0; j < cv.cw / 8; j++) {
        const YkPxClip k = yk_wpx_clip(j, d, ww);
        if (k.n < 0 || k.n > 8) FAIL("clip of column %d keeps %d", j, k.n);
        if (k.n == 0) continue;
        if (k.src0 < 0 || k.src0 + k.n > 8) FAIL("clip of column %d reads %d..%d of its segment", j, k.src0, k.src0 + k.n - 1);
        if (k.dst < 0 || k.dst + k.n > ww) FAIL("clip of column %d writes %d..%d", j, k.dst, k.dst + k.n - 1);
        for (int i = 0; i < k.n; i++) {
            const int src = cv.c0 + 8 * j + k.src0 + i;                     // image column read
            if (src < cv.c0 || src >= cv.c0 + cv.cw || src >= w) FAIL("column %d reads image column %d outside the cover", j, src);
            if (src != x0 + k.dst + i) FAIL("column %d puts image column %d at window column %d", j, src, k.dst + i);
            seen[(size_t)(k.dst + i)]++;
        }
    }
    for (int i = 0; i < ww; i++)
        if (seen[(size_t)i] != 1) FAIL("window column %d is written %d times", i, seen[(size_t)i]);
    return true;
}

static bool check_window(int w, int x0, int ww) {
    const YkPxCover c = yk_wpx_cover(x0, ww);
    if ((c.c0 | c.cw) & 7) FAIL("single cover %d+%d is not 8-aligned", c.c0, c.cw);
    if (c.c0 < 0 || c.cw < 8 || c.c0 + c.cw > w) FAIL("single cover %d+%d leaves the image", c.c0, c.cw);
    if (c.c0 > x0 || c.c0 + c.cw < x0 + ww) FAIL("single cover %d+%d misses the window", c.c0, c.cw);
    if (x0 - c.c0 >= 8 || c.c0 + c.cw - (x0 + ww) >= 8) FAIL("single cover %d+%d is not minimal", c.c0, c.cw);
    const YkPxCover s = yk_wpx_shared_cover(x0, ww, w);
    if (s.cw != yk_wpx_shared_size(ww, w)) FAIL("shared cover size %d depends on x0", s.cw);
    if ((s.c0 | s.cw) & 7) FAIL("shared cover %d+%d is not 8-aligned", s.c0, s.cw);
    if (s.c0 < 0 || s.cw < 8 || s.c0 + s.cw > w) FAIL("shared cover %d+%d leaves the image", s.c0, s.cw);
    if (s.c0 > x0 || s.c0 + s.cw < x0 + ww) FAIL("shared cover %d+%d misses the window", s.c0, s.cw);
    if (s.cw - ww >= 16) FAIL("shared cover size %d is 16 or more above the window", s.cw);
    return check_clip(w, x0, ww, c) && check_clip(w, x0, ww, s);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: window_px_tool check <w> | show <w> <x0> <ww>\n"); return 2; }
    const int w = atoi(argv[2]);
    if (w < 8 || (w & 7) || w > 32760) { fprintf(stderr, "bad image size\n"); return 2; }
    if (!strcmp(argv[1], "check") && argc == 3) {
        long n = 0;
        for (int ww = -1; ww <= w + 1; ww++)
            for (int x0 = -1; x0 <= w; x0++) {
                const bool inside = x0 >= 0 && ww >= 1 && (long)x0 + ww <= w;          // the rule, spelled out
                if (yk_wpx_axis_ok(x0, ww, w) != inside) { printf("FAIL w=%d x0=%d ww=%d: the rule says %d\n", w, x0, ww, (int)!inside); return 1; }
                if (!inside) continue;
                if (!check_window(w, x0, ww)) return 1;
                n++;
            }
        const int big = 0x7fffffff;                                                  // no overflow at the far end of int
        if (yk_wpx_axis_ok(big, big, w) || yk_wpx_axis_ok(1, big, w) || yk_wpx_axis_ok(big, 1, w)) { printf("FAIL w=%d: the rule overflows\n", w); return 1; }
        printf("ok %ld\n", n);
        return 0;
    }
    if (!strcmp(argv[1], "show") && argc == 5) {
        const int x0 = atoi(argv[3]), ww = atoi(argv[4]);
        if (!yk_wpx_axis_ok(x0, ww, w)) { printf("bad\n"); return 3; }
        const YkPxCover c = yk_wpx_cover(x0, ww), s = yk_wpx_shared_cover(x0, ww, w);
        printf("%d %d %d %d :", c.c0, c.cw, s.c0, s.cw);
        for (int j = 0; j < s.cw / 8; j++) {
            const YkPxClip k = yk_wpx_clip(j, x0 - s.c0, ww);
            printf(" %d,%d,%d,%d", j, k.src0, k.n, k.dst);
        }
        printf("\n");
        return 0;
    }
    fprintf(stderr, "usage: window_px_tool check <w> | show <w> <x0> <ww>\n");
    return 2;
}
