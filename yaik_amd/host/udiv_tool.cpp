// CPU-only check of the multiply-and-shift division the fused encode kernel's unit decode uses (../csrc/yk_udiv.h): the same
// yk_udiv_make / yk_udiv the library compiles, compared with the machine's division.  Prints one JSON line.
//   udiv_tool all    <dMax> <factor>        every divisor d in 1..dMax with every numerator in [0, d * factor)
//   udiv_tool ranges <dMax> <seed> <nRand>  every divisor d in 1..dMax with the end points of its quotient ranges (k d - 1, k d for k = 1, 2,
//                                           3, 1023, 1024, 1025 and the last k below the limit), 0, 1, the limit's last two numerators, and
//                                           nRand seeded numerators in [0, YK_UDIV_LIMIT)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../csrc/yk_udiv.h"

static uint64_t checked = 0, bad = 0, firstD = 0, firstN = 0;
static inline void check(uint32_t n, uint32_t d, const YkUdiv& r) {
    checked++;
    if (yk_udiv(n, r.mul, r.shift) != n / d) { if (!bad) { firstD = d; firstN = n; } bad++; }
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: udiv_tool all <dMax> <factor> | ranges <dMax> <seed> <nRand>\n"); return 2; }
    const uint32_t dMax = (uint32_t)strtoul(argv[2], nullptr, 10);
    uint64_t maxN = 0;
    if (!strcmp(argv[1], "all")) {
        const uint64_t factor = strtoull(argv[3], nullptr, 10);
        for (uint32_t d = 1; d <= dMax; d++) {
            const YkUdiv r = yk_udiv_make(d);
            const uint64_t end = (uint64_t)d * factor;
            if (end > YK_UDIV_LIMIT) { fprintf(stderr, "d * factor beyond the limit\n"); return 2; }
            for (uint32_t n = 0; n < (uint32_t)end; n++) check(n, d, r);
            if (end - 1 > maxN) maxN = end - 1;
        }
    } else if (!strcmp(argv[1], "ranges") && argc >= 5) {
        uint64_t rng = strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
        const int nRand = atoi(argv[4]);
        const uint64_t lim = YK_UDIV_LIMIT;
        for (uint32_t d = 1; d <= dMax; d++) {
            const YkUdiv r = yk_udiv_make(d);
            const uint64_t ks[7] = { 1, 2, 3, 1023, 1024, 1025, (lim - 1) / d };
            for (uint64_t k : ks) {
                const uint64_t a = k * d;
                if (a - 1 < lim) check((uint32_t)(a - 1), d, r);
                if (a < lim) check((uint32_t)a, d, r);
            }
            check(0u, d, r); check(1u, d, r); check((uint32_t)(lim - 1), d, r); check((uint32_t)(lim - 2), d, r);
            for (int i = 0; i < nRand; i++) {
                rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;                          // xorshift64
                check((uint32_t)(rng % lim), d, r);
            }
        }
        maxN = lim - 1;
    } else { fprintf(stderr, "unknown mode\n"); return 2; }
    printf("{\"mode\": \"%s\", \"dMax\": %u, \"limit\": %u, \"maxNumerator\": %" PRIu64 ", \"checked\": %" PRIu64 ", \"mismatches\": %" PRIu64
           ", \"firstBad\": [%" PRIu64 ", %" PRIu64 "]}\n", argv[1], dMax, (unsigned)YK_UDIV_LIMIT, maxN, checked, bad, firstD, firstN);
    return bad ? 1 : 0;
}
