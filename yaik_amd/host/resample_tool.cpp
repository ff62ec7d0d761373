// CPU-only: the arithmetic of the resampled outputs (yaik_amd/csrc/yk_resample.h, no HIP linked), for the `not gpu` tests.
//   resample_tool check                      every (n_src, n_out) in 1..40 x 1..40 and (16384, 1), (1, 16384), (16384, 16384), (16383, 224): every tap
//                                            against a 64-bit form and against the rational position, no intermediate outside int32, and the blend
//                                            against a 64-bit form: prints "ok <cases checked>", or the first failure and exit status 1
//   resample_tool taps <n_src> <n_out>       "<step>,<off>" then "<i0>,<i1>,<f>" for every output index
//   resample_tool blend <a> <b> <c> <d> <fx> <fy>     the value
//   resample_tool cover <x0> <y0> <sw> <sh>  "<x0>,<y0>,<x1>,<y1>" of the rectangle's own cover
//   resample_tool ok <x0> <y0> <sw> <sh> <w> <h> <ow> <oh>     "1" if yk_rs_rect_ok takes them, else "0"
//   resample_tool words <x0> <y0> <sw> <sh> <ow> <oh> <mirror>    the nine words of a frame
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../csrc/yk_resample.h"

typedef long long i64;
static const i64 I32MAX = 2147483647LL;
static bool in32(i64 v) { return v >= -I32MAX - 1 && v <= I32MAX; }

#define FAIL(...) do { printf("FAIL n_src=%d n_out=%d: ", ns, no); printf(__VA_ARGS__); printf("\n"); return false; } while (0)

static bool check_pair(int ns, int no, long* n) {
    const YkRsAxis ax = yk_rs_axis(ns, no);
    const i64 S = ((i64)ns << 16), step = S / no, off = (step >> 1) - 32768;
    if (!in32(S) || ax.step != step || ax.off != off) FAIL("axis {%d, %d}, 64-bit {%lld, %lld}", ax.step, ax.off, step, off);
    if ((i64)(int)((unsigned)ns << 16) / no != step) FAIL("step needs more than 32 bits");
    const i64 last = ns - 1;
    for (int i = 0; i < no; i++) {
        const i64 raw = off + (i64)i * step;
        if (!in32((i64)i * step) || !in32(raw) || !in32(last << 16)) FAIL("output %d leaves int32", i);
        // the rational position: E = (i + 0.5) * n_src / n_out * 65536; the truncations of step and of step / 2 keep raw + 32768 in (E - (i + 1), E]
        const i64 lhs = 2 * (i64)no * (raw + 32768), E2 = (2 * (i64)i + 1) * S;
        if (lhs > E2 || lhs + 2 * (i64)no * (i + 1) <= E2) FAIL("output %d: position %lld is not within i + 1 below the exact one", i, raw);
        i64 pos = raw < 0 ? 0 : raw;
        if (pos > (last << 16)) pos = last << 16;
        const i64 i0 = pos >> 16, f = (pos >> 8) & 255, i1 = i0 + 1 < ns ? i0 + 1 : last;
        const YkRsTap t = yk_rs_tap(ax, i, ns);
        if (t.i0 != i0 || t.i1 != i1 || t.f != f) FAIL("output %d: tap {%d, %d, %d}, 64-bit {%lld, %lld, %lld}", i, t.i0, t.i1, t.f, i0, i1, f);
        if (t.i0 < 0 || t.i1 >= ns || t.i1 < t.i0 || t.i1 > t.i0 + 1 || t.f < 0 || t.f > 255) FAIL("output %d: tap {%d, %d, %d} leaves the source", i, t.i0, t.i1, t.f);
        if (t.i0 == last && t.f != 0 && raw >= (last << 16)) FAIL("output %d: a clamped position keeps a fraction", i);
        ++*n;
    }
    if (ns == no)                                                   // identity: every tap is its own pixel with no fraction
        for (int i = 0; i < no; i++) { const YkRsTap t = yk_rs_tap(ax, i, ns); if (t.i0 != i || t.f != 0) FAIL("identity: output %d reads %d + %d/256", i, t.i0, t.f); }
    if (ns == 2 * no)                                               // 2x: the pair 2i, 2i + 1 at one half
        for (int i = 0; i < no; i++) { const YkRsTap t = yk_rs_tap(ax, i, ns); if (t.i0 != 2 * i || t.i1 != 2 * i + 1 || t.f != 128) FAIL("2x: output %d reads %d, %d + %d/256", i, t.i0, t.i1, t.f); }
    return true;
}

static bool check_blend(long* n) {
    static const int vals[] = { 0, 1, 2, 127, 128, 129, 254, 255 };
    for (int a : vals) for (int b : vals) for (int c : vals) for (int d : vals)
        for (int fx = 0; fx < 256; fx += (fx < 4 || fx > 250 || (fx > 125 && fx < 131)) ? 1 : 7)
            for (int fy = 0; fy < 256; fy += (fy < 4 || fy > 250 || (fy > 125 && fy < 131)) ? 1 : 7) {
                const i64 top = (i64)a * (256 - fx) + (i64)b * fx, bot = (i64)c * (256 - fx) + (i64)d * fx;
                const i64 acc = top * (256 - fy) + bot * fy + 32768, v = acc >> 16;
                const int got = yk_rs_blend(a, b, c, d, fx, fy);
                if (!in32(acc) || got != v || got < 0 || got > 255) { printf("FAIL blend %d %d %d %d %d %d: %d, 64-bit %lld\n", a, b, c, d, fx, fy, got, v); return false; }
                if (a == b && b == c && c == d && got != a) { printf("FAIL blend of a constant %d gives %d\n", a, got); return false; }
                if (fx == 128 && fy == 128 && got != ((a + b + c + d + 2) >> 2)) { printf("FAIL blend at one half is not the box mean, halves up\n"); return false; }
                if (fx == 0 && fy == 0 && got != a) { printf("FAIL blend without fractions is not a\n"); return false; }
                ++*n;
            }
    return true;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "check")) {
        long n = 0;
        for (int ns = 1; ns <= 40; ns++)
            for (int no = 1; no <= 40; no++)
                if (!check_pair(ns, no, &n)) return 1;
        static const int big[4][2] = { { 16384, 1 }, { 1, 16384 }, { 16384, 16384 }, { 16383, 224 } };
        for (auto& p : big)
            if (!check_pair(p[0], p[1], &n)) return 1;
        if (!check_blend(&n)) return 1;
        printf("ok %ld\n", n);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "taps")) {
        const int ns = atoi(argv[2]), no = atoi(argv[3]);
        if (ns < 1 || no < 1 || ns > YK_RS_MAX || no > YK_RS_MAX) { printf("bad\n"); return 3; }
        const YkRsAxis ax = yk_rs_axis(ns, no);
        printf("%d,%d", ax.step, ax.off);
        for (int i = 0; i < no; i++) { const YkRsTap t = yk_rs_tap(ax, i, ns); printf(" %d,%d,%d", t.i0, t.i1, t.f); }
        printf("\n");
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "blend")) {
        int v[6];
        for (int k = 0; k < 6; k++) v[k] = atoi(argv[2 + k]);
        for (int k = 0; k < 6; k++) if (v[k] < 0 || v[k] > 255) { printf("bad\n"); return 3; }
        printf("%d\n", yk_rs_blend(v[0], v[1], v[2], v[3], v[4], v[5]));
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "cover")) {
        const YkRsCover c = yk_rs_cover(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
        printf("%d,%d,%d,%d\n", c.x0, c.y0, c.x1, c.y1);
        return 0;
    }
    if (argc == 10 && !strcmp(argv[1], "ok")) {
        int v[8];
        for (int k = 0; k < 8; k++) v[k] = atoi(argv[2 + k]);
        printf("%d\n", (int)yk_rs_rect_ok(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]));
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "words")) {
        int v[7], t[YK_RS_WORDS];
        for (int k = 0; k < 7; k++) v[k] = atoi(argv[2 + k]);
        if (v[2] < 1 || v[3] < 1 || !yk_rs_size_ok(v[4], v[5]) || v[2] > YK_RS_MAX || v[3] > YK_RS_MAX) { printf("bad\n"); return 3; }
        yk_rs_words(v[0], v[1], v[2], v[3], v[4], v[5], v[6], t);
        for (int k = 0; k < YK_RS_WORDS; k++) printf("%s%d", k ? "," : "", t[k]);
        printf("\n");
        return 0;
    }
    fprintf(stderr, "usage: resample_tool check | taps <n_src> <n_out> | blend <a> <b> <c> <d> <fx> <fy> | cover <x0> <y0> <sw> <sh> | ok <x0> <y0> <sw> <sh> <w> <h> <ow> <oh> | words ...\n");
    return 2;
}
