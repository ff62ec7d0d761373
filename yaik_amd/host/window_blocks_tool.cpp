// CPU-only: the block list of yk_decode_render_windows_device for windows given on the command line (no HIP linked), for the `not gpu` tests.
//   window_blocks_tool <w> <h> <ww> <wh> [-d <id>[,<id>...]] [-r <calls>] <x0> <y0> [<x0> <y0> ...]
//   -d: blocks that count as rendered before the first call;  -r: the same windows again, <calls> times in all (default 1)
//   one line per call:  <rendered> <total> : <id> <id> ...        (the ids the call would render, ascending)
//   windows that break the rule of yk_decode_set_window:  "bad" and exit status 3, nothing else printed
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../csrc/yk_window_blocks.h"

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: window_blocks_tool <w> <h> <ww> <wh> [-d ids] [-r calls] <x0> <y0>...\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), ww = atoi(argv[3]), wh = atoi(argv[4]);
    if (w < 8 || h < 8 || (w & 7) || (h & 7) || w > 32760 || h > 32760) { fprintf(stderr, "bad image size\n"); return 2; }
    YkWindowBlocks B;
    yk_wb_reset(B, w, h);
    int calls = 1, i = 5;
    for (; i + 1 < argc && argv[i][0] == '-' && (argv[i][1] == 'd' || argv[i][1] == 'r') && !argv[i][2]; i += 2) {
        if (argv[i][1] == 'r') { calls = atoi(argv[i + 1]); continue; }
        for (char* p = argv[i + 1]; *p;) {
            const long id = strtol(p, &p, 10);
            if (id < 0 || id >= yk_wb_total(B)) { fprintf(stderr, "block id out of range\n"); return 2; }
            if (!(B.done[(size_t)id >> 6] >> (id & 63) & 1)) { B.done[(size_t)id >> 6] |= (uint64_t)1 << (id & 63); B.rendered++; }
            if (*p == ',') p++;
        }
    }
    if ((argc - i) < 2 || ((argc - i) & 1)) { fprintf(stderr, "window origins come in pairs\n"); return 2; }
    std::vector<int> xy;
    for (; i < argc; i++) xy.push_back(atoi(argv[i]));
    const int n = (int)(xy.size() / 2);
    if (n > 1024 || !yk_wb_windows_ok(B, n, xy.data(), ww, wh)) { printf("bad\n"); return 3; }
    std::vector<uint32_t> list;
    for (int c = 0; c < calls; c++) {
        yk_wb_take(B, n, xy.data(), ww, wh, list);
        printf("%d %d :", B.rendered, yk_wb_total(B));
        for (uint32_t id : list) printf(" %u", id);
        printf("\n");
    }
    return 0;
}
