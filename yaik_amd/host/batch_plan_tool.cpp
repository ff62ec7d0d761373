// CPU-only: the plan of YAIK_DecodeImagesToDevice for a list of .yaik files, one line per file (no HIP linked), for the `not gpu` tests.
//   batch_plan_tool <a.yaik> [<b.yaik> ...]
//   <index> batchable <w> <h> mip=<0|1> alpha=<mode|-1> passes=<i,j,..|-> d1=<0|1>
//   <index> fallback <w> <h> <the rule it broke>
//   <index> mismatch <w> <h>            a readable header of another size than file 0's
//   <index> badheader
#include <cstdio>
#include <vector>
#include "batch_plan.h"

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: batch_plan_tool <file.yaik>...\n"); return 2; }
    int w0 = 0, h0 = 0;
    for (int i = 1; i < argc; i++) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
        std::vector<uint8_t> s((size_t)n);
        if (n && fread(s.data(), 1, (size_t)n, f) != (size_t)n) { fclose(f); return 2; }
        fclose(f);
        int w = 0, h = 0; bool rgba = false;
        if (yaikplan::readHeader(s.data(), (uint32_t)n, &w, &h, &rgba) != 0) { printf("%d badheader\n", i - 1); continue; }
        if (i == 1) { w0 = w; h0 = h; }
        if (w != w0 || h != h0) { printf("%d mismatch %d %d\n", i - 1, w, h); continue; }
        yaikplan::StreamPlan p;
        if (!yaikplan::planStream(s.data(), (uint32_t)n, p)) { printf("%d fallback %d %d %s\n", i - 1, w, h, p.why); continue; }
        printf("%d batchable %d %d mip=%d alpha=%d passes=", i - 1, w, h, p.hasMip ? 1 : 0, p.alphaMode);
        bool any = false;
        for (int k = 0; k < yaikplan::NUM_PASSES; k++) if (p.grad[k].present) { printf(any ? ",%d" : "%d", k); any = true; }
        printf("%s d1=%d\n", any ? "" : "-", p.has1d ? 1 : 0);
    }
    return 0;
}
