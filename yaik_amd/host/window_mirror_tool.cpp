// CPU-only: the clip-and-mirror arithmetic of the normalising de-tile (yaik_amd/csrc/yk_window_mirror.h, no HIP linked), for the `not gpu` tests.
//   window_mirror_tool check <dmax> <wwmax>    every offset d = 0..dmax, window length ww = 1..wwmax, mirror 0 and 1, every tile column of a cover
//                                              of d + ww pixels and two columns beyond it, against a brute-force enumeration:
//                                              prints "ok <cases checked>", or the first failure and exit status 1
//   window_mirror_tool show <d> <ww> <mirror>  "<j>,<src0>,<n>,<dst>,<reversed src0>" for every tile column j of the cover
//   window_mirror_tool param <float as hex bits>   "1" if yk_norm_param_ok takes the value, else "0"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../csrc/yk_window_mirror.h"

#define FAIL(...) do { printf("FAIL d=%d ww=%d mirror=%d: ", d, ww, mirror); printf(__VA_ARGS__); printf("\n"); return false; } while (0)

static bool check(int d, int ww, int mirror) {
    // brute force: cover column d + x is window column x, which lands at destination column x, or ww - 1 - x mirrored
    std::vector<int> want((size_t)ww), got((size_t)ww, -1), gotRev((size_t)ww, -1);
    for (int x = 0; x < ww; x++) want[(size_t)(mirror ? ww - 1 - x : x)] = d + x;
    const int nCols = (d + ww + 7) / 8 + 2;
    for (int j = 0; j < nCols; j++) {
        const YkPxMirrorClip k = yk_wpx_clip_mirror(j, d, ww, mirror);
        if (k.n < 0 || k.n > 8) FAIL("column %d keeps %d", j, k.n);
        if (k.n == 0) continue;
        if (k.src0 < 0 || k.src0 + k.n > 8) FAIL("column %d reads %d..%d of its segment", j, k.src0, k.src0 + k.n - 1);
        if (k.dst < 0 || k.dst + k.n > ww) FAIL("column %d writes %d..%d", j, k.dst, k.dst + k.n - 1);
        const int r0 = yk_wpx_mirror_src0(k, mirror);
        if (r0 < 0 || r0 + k.n > 8) FAIL("column %d reads %d..%d of its reversed segment", j, r0, r0 + k.n - 1);
        for (int i = 0; i < k.n; i++) {
            // the header's own statement of the mapping
            const int to = mirror ? k.dst + k.n - 1 - i : k.dst + i;
            if (got[(size_t)to] != -1) FAIL("destination column %d is written twice", to);
            got[(size_t)to] = 8 * j + k.src0 + i;
            // what the kernel does: reverse the segment (column c -> 7 - c), then store the kept columns in rising order from dst
            const int c = r0 + i, orig = mirror ? 7 - c : c;
            if (gotRev[(size_t)(k.dst + i)] != -1) FAIL("destination column %d is written twice (reversed form)", k.dst + i);
            gotRev[(size_t)(k.dst + i)] = 8 * j + orig;
        }
    }
    for (int x = 0; x < ww; x++) {
        if (got[(size_t)x] != want[(size_t)x]) FAIL("destination column %d holds cover column %d, not %d", x, got[(size_t)x], want[(size_t)x]);
        if (gotRev[(size_t)x] != want[(size_t)x]) FAIL("destination column %d holds cover column %d, not %d (reversed form)", x, gotRev[(size_t)x], want[(size_t)x]);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "check")) {
        const int dmax = atoi(argv[2]), wwmax = atoi(argv[3]);
        if (dmax < 0 || dmax > 4096 || wwmax < 1 || wwmax > 4096) { fprintf(stderr, "bad range\n"); return 2; }
        long n = 0;
        for (int d = 0; d <= dmax; d++)
            for (int ww = 1; ww <= wwmax; ww++)
                for (int mirror = 0; mirror < 2; mirror++) {
                    if (!check(d, ww, mirror)) return 1;
                    n++;
                }
        printf("ok %ld\n", n);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "show")) {
        const int d = atoi(argv[2]), ww = atoi(argv[3]), mirror = atoi(argv[4]);
        if (d < 0 || ww < 1) { printf("bad\n"); return 3; }
        for (int j = 0; j < (d + ww + 7) / 8; j++) {
            const YkPxMirrorClip k = yk_wpx_clip_mirror(j, d, ww, mirror);
            printf("%s%d,%d,%d,%d,%d", j ? " " : "", j, k.src0, k.n, k.dst, yk_wpx_mirror_src0(k, mirror));
        }
        printf("\n");
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "param")) {
        const uint32_t bits = (uint32_t)strtoul(argv[2], nullptr, 16);
        float v;
        memcpy(&v, &bits, 4);
        printf("%d\n", (int)yk_norm_param_ok(v));
        return 0;
    }
    fprintf(stderr, "usage: window_mirror_tool check <dmax> <wwmax> | show <d> <ww> <mirror> | param <hex bits>\n");
    return 2;
}
