// yk_palette.hip — PaletteCompressor (encoder/EncoderContext.cpp:3259-3502; host form: yaik_amd/host/palette.cpp) on the GPU, byte-exact.
//
// The work is a list of SEGMENTS (device pointer, colours): the seven passes of a frame and the 7 x N streams of a batch are the same problem, and
// every kernel below is launched once over all segments of a call.  Per call, all on the handle's stream and without a host synchronisation in between:
//   clear       the vote tables (two memsets)
//   vote        a workgroup stages 256 colours + the 65 in front of them in LDS; a thread finds the nearest of its 64 predecessors (first minimum),
//               the workgroup combines its votes in an LDS hash and sends ONE update per distinct delta to the segment's table in HBM
//               (votes, smallest voting n = registration order).  Votes for (0,0,0) are dropped: row 0 is fixed and its count is never read.
//   select 1    a workgroup per slice of 16384 table slots: the slice's 128 best (votes descending, first n ascending) and its occupied slots
//   select 2    a workgroup per segment: the 127 best over its slices, sorted, and the row count
//   chain       a wave per run of `chain` segments walks them in order and writes each segment's 64-row find table (stale rows included)
//   token       a thread per colour: the find table as an LDS hash "delta -> lowest row", the 65 predecessors from the same staging; one packed
//               token (1..4 bytes) per colour and the bytes per workgroup
//   scan        a workgroup per segment: header length + exclusive prefix of the workgroups' bytes, the payload length
//   layout      one workgroup: payload offsets, each a multiple of 16
//   emit        header + token bytes at their offsets
// and then ONE blocking read-back: the payload lengths and offsets (8 bytes per segment).
//
// No overflow path.  PaletteCompressor caps its output at 3 * size = 9 * entries bytes.  A stream of e >= 1 colours has rows <= min(e, 128) (row 0
// plus at most e - 1 voted deltas), so header = 1 + 3 * rows + 3 <= 4 + 3 * e bytes, and at most 4 bytes per further colour: 4 + 3e + 4(e - 1) = 7e
// bytes at most, against 9e.  The cap cannot be reached for a length that is a multiple of 3, and the payload buffer reserves 7 bytes per colour.
#include "yk_common.h"

#define PAL_WG    256                       // colours per workgroup = threads per workgroup
#define PAL_BACK  65                        // colours staged in front of a workgroup's own
#define PAL_SLICE 16384u                    // vote-table slots per workgroup of the first selection stage
#define PAL_KEY0  (256u | (256u << 10) | (256u << 20))      // the packed delta (0,0,0); a packed delta is never 0, which marks an empty slot
#define PAL_MAX_COLOURS (1u << 28)          // per call: every offset below fits 32 bits
#define PAL_MAX_SEGS    65536

struct YkPalSeg {
    const uint8_t* src;
    uint32_t n;                             // colours
    uint32_t wg0;                           // first workgroup of the colour grid
    uint32_t tabOff, tabCap;                // the segment's vote table: slots [tabOff, tabOff + tabCap)
    uint32_t slice0;                        // first workgroup of the first selection stage
    uint32_t colOff;                        // first colour's token
};

struct YkPalBufs {
    const YkPalSeg* segs; uint32_t nSeg;
    uint32_t* tKey; uint32_t* tVotes; uint32_t* tFirst;                 // vote tables of all segments
    unsigned long long* candKey; uint32_t* candDelta; uint32_t* sliceCnt;   // [slices][128], [slices]
    uint32_t* book;                         // [nSeg][128]: [0] = rows, [i] = row i's packed delta (1..127), sorted
    uint32_t* find;                         // [nSeg][64]
    uint32_t* tok;                          // a packed token per colour
    uint32_t* wgBytes; uint32_t* wgOff;     // per workgroup of the colour grid
    uint32_t* segLen; uint32_t* segBase;    // [nSeg], [nSeg] (contiguous: one read-back)
};

// the last segment whose first workgroup (or slice) is <= i: empty segments own no workgroup and are never found
template <bool SLICES> __device__ inline uint32_t pal_find_seg(const YkPalSeg* __restrict__ segs, uint32_t nSeg, uint32_t i) {
    uint32_t lo = 0, hi = nSeg - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        const uint32_t first = SLICES ? segs[mid].slice0 : segs[mid].wg0;
        if (first <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline uint32_t pal_hash(uint32_t key) { uint32_t h = key * 0x9E3779B1u; return h ^ (h >> 15); }
__device__ inline uint32_t pal_delta_key(uint32_t a, uint32_t b) {     // a - b per channel, each in -255..255, not reduced mod 256
    const int dr = (int)(a & 255u) - (int)(b & 255u), dg = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u), db = (int)((a >> 16) & 255u) - (int)((b >> 16) & 255u);
    return (uint32_t)(dr + 256) | ((uint32_t)(dg + 256) << 10) | ((uint32_t)(db + 256) << 20);
}

// LDS staging: col[i] = colour base - 65 + i as r | g << 8 | b << 16 (0 outside the stream)
__device__ inline void pal_stage(uint32_t* col, const uint8_t* __restrict__ src, uint32_t n, uint32_t base, uint32_t t) {
    for (uint32_t i = t; i < PAL_WG + PAL_BACK; i += PAL_WG) {
        const long long k = (long long)base - PAL_BACK + i;
        uint32_t v = 0;
        if (k >= 0 && k < (long long)n) { const uint8_t* p = src + (size_t)k * 3; v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }
        col[i] = v;
    }
}

__device__ inline uint32_t pal_block_excl(uint32_t v, uint32_t* sh, uint32_t t, uint32_t* total) {       // 256 threads
    sh[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < PAL_WG; off <<= 1) {
        const uint32_t x = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint32_t incl = sh[t];
    *total = sh[PAL_WG - 1];
    __syncthreads();
    return incl - v;
}

// ---- votes ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PAL_WG) void yk_pal_vote_kernel(YkPalBufs B) {
    __shared__ uint32_t col[PAL_WG + PAL_BACK];
    __shared__ uint32_t lKey[512], lVotes[512], lFirst[512];
    const uint32_t t = threadIdx.x, wg = blockIdx.x;
    const YkPalSeg S = B.segs[pal_find_seg<false>(B.segs, B.nSeg, wg)];
    const uint32_t base = (wg - S.wg0) * PAL_WG, n = base + t;
    pal_stage(col, S.src, S.n, base, t);
    for (uint32_t i = t; i < 512; i += PAL_WG) { lKey[i] = 0; lVotes[i] = 0; lFirst[i] = 0xFFFFFFFFu; }
    __syncthreads();
    if (n >= 1 && n < S.n) {
        const uint32_t me = col[t + PAL_BACK];
        const int mr = (int)(me & 255u), mg = (int)((me >> 8) & 255u), mb = (int)((me >> 16) & 255u);
        uint32_t best = 0xFFFFFFFFu;                                    // distance << 6 | ordinal: distance <= 3 * 255^2 < 2^18, the first minimum wins
        for (uint32_t k = n >= 64 ? 0u : 64u - n; k < 64; k++) {        // prev = n - 64 + k
            const uint32_t p = col[t + 1 + k];
            const int dr = mr - (int)(p & 255u), dg = mg - (int)((p >> 8) & 255u), db = mb - (int)((p >> 16) & 255u);
            best = min(best, ((uint32_t)(dr * dr + dg * dg + db * db) << 6) | k);
        }
        const uint32_t key = pal_delta_key(me, col[t + 1 + (best & 63u)]);
        if (key != PAL_KEY0) {
            uint32_t h = pal_hash(key) >> 23;                           // 256 inserts into 512 slots: always ends
            for (;;) {
                const uint32_t old = atomicCAS(&lKey[h], 0u, key);
                if (old == 0u || old == key) { atomicAdd(&lVotes[h], 1u); atomicMin(&lFirst[h], n); break; }
                h = (h + 1) & 511u;
            }
        }
    }
    __syncthreads();
    for (uint32_t i = t; i < 512; i += PAL_WG) {                        // one update per distinct delta of the workgroup
        const uint32_t key = lKey[i];
        if (!key) continue;
        uint32_t s = __umulhi(pal_hash(key), S.tabCap);                 // tabCap > 1.5 x the deltas a segment can hold: always ends
        for (;;) {
            const uint32_t old = atomicCAS(&B.tKey[S.tabOff + s], 0u, key);
            if (old == 0u || old == key) { atomicAdd(&B.tVotes[S.tabOff + s], lVotes[i]); atomicMin(&B.tFirst[S.tabOff + s], lFirst[i]); break; }
            if (++s == S.tabCap) s = 0;
        }
    }
}

// ---- row selection: the 128 largest 64-bit keys of a sequence of candidates, by one workgroup ------------------------------------------------
// key = votes << 32 | ~first n: votes descending, registration order ascending; distinct deltas of a segment have distinct first n, so keys are unique
struct PalTop { unsigned long long key[512]; uint32_t delta[512]; uint32_t nPend; unsigned long long thr; };

__device__ inline void pal_top_init(PalTop& T, uint32_t t) {
    for (uint32_t i = t; i < 512; i += PAL_WG) { T.key[i] = 0; T.delta[i] = 0; }
    if (t == 0) { T.nPend = 0; T.thr = 0; }
    __syncthreads();
}
// sorts [best 128 | pending | zeros] descending (bitonic, one pair per thread and step), keeps the first 128
__device__ inline void pal_top_flush(PalTop& T, uint32_t t) {
    const uint32_t cnt = 128u + T.nPend;
    __syncthreads();
    for (uint32_t i = t; i < 512; i += PAL_WG) if (i >= cnt) { T.key[i] = 0; T.delta[i] = 0; }
    __syncthreads();
    for (uint32_t k = 2; k <= 512; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
            const unsigned long long a = T.key[i], b = T.key[l];
            if (((i & k) == 0) ? a < b : a > b) {
                const uint32_t da = T.delta[i], db = T.delta[l];
                T.key[i] = b; T.key[l] = a; T.delta[i] = db; T.delta[l] = da;
            }
            __syncthreads();
        }
    if (t == 0) { T.nPend = 0; T.thr = T.key[127]; }
    __syncthreads();
}
// every thread of the workgroup offers one candidate (key 0 = none); at most 128 are pending on entry, at most 384 afterwards
__device__ inline void pal_top_offer(PalTop& T, uint32_t t, unsigned long long key, uint32_t delta) {
    if (key > T.thr) { const uint32_t pos = 128u + atomicAdd(&T.nPend, 1u); T.key[pos] = key; T.delta[pos] = delta; }
    __syncthreads();
    const uint32_t pend = T.nPend;
    __syncthreads();
    if (pend > 128u) pal_top_flush(T, t);
}

__global__ __launch_bounds__(PAL_WG) void yk_pal_select1_kernel(YkPalBufs B) {
    __shared__ PalTop T;
    __shared__ uint32_t occupied;
    const uint32_t t = threadIdx.x, sl = blockIdx.x;
    const YkPalSeg S = B.segs[pal_find_seg<true>(B.segs, B.nSeg, sl)];
    const uint32_t lo = (sl - S.slice0) * PAL_SLICE, hi = min(S.tabCap, lo + PAL_SLICE);
    if (t == 0) occupied = 0;
    pal_top_init(T, t);
    uint32_t mine = 0;
    for (uint32_t s0 = lo; s0 < hi; s0 += PAL_WG) {                     // uniform trip count
        const uint32_t s = s0 + t;
        unsigned long long key = 0; uint32_t delta = 0;
        if (s < hi) {
            delta = B.tKey[S.tabOff + s];
            if (delta) { mine++; key = ((unsigned long long)B.tVotes[S.tabOff + s] << 32) | (0xFFFFFFFFu - B.tFirst[S.tabOff + s]); }
        }
        pal_top_offer(T, t, key, delta);
    }
    pal_top_flush(T, t);
    if (mine) atomicAdd(&occupied, mine);
    __syncthreads();
    if (t < 128) { B.candKey[(size_t)sl * 128 + t] = T.key[t]; B.candDelta[(size_t)sl * 128 + t] = T.delta[t]; }
    if (t == 0) B.sliceCnt[sl] = occupied;
}

__global__ __launch_bounds__(PAL_WG) void yk_pal_select2_kernel(YkPalBufs B) {
    __shared__ PalTop T;
    __shared__ uint32_t distinct;
    const uint32_t t = threadIdx.x, sg = blockIdx.x;
    const YkPalSeg S = B.segs[sg];
    if (S.n == 0) return;
    const uint32_t nSl = (S.tabCap + PAL_SLICE - 1) / PAL_SLICE;
    if (t == 0) distinct = 0;
    pal_top_init(T, t);
    uint32_t mine = 0;
    for (uint32_t i = t; i < nSl; i += PAL_WG) mine += B.sliceCnt[S.slice0 + i];
    const uint32_t nCand = nSl * 128u;
    for (uint32_t c0 = 0; c0 < nCand; c0 += PAL_WG) {
        const uint32_t i = c0 + t;
        unsigned long long key = 0; uint32_t delta = 0;
        if (i < nCand) { key = B.candKey[(size_t)S.slice0 * 128 + i]; delta = B.candDelta[(size_t)S.slice0 * 128 + i]; }
        pal_top_offer(T, t, key, delta);
    }
    pal_top_flush(T, t);
    if (mine) atomicAdd(&distinct, mine);
    __syncthreads();
    uint32_t* book = B.book + (size_t)sg * 128;
    if (t == 0) book[0] = 1u + distinct;                                // row 0 = (0,0,0), registered first
    else if (t < 128) book[t] = T.delta[t - 1];                         // 0 beyond the rows: never read
}

// ---- book chaining: rows 0..63 of the table FindCodeBook scans, stale or not -------------------------------------------------------------------
__global__ __launch_bounds__(64) void yk_pal_chain_kernel(YkPalBufs B, uint32_t runLen, uint32_t* carry, int carryIn, int carryOut) {
    const uint32_t t = threadIdx.x, s0 = blockIdx.x * runLen, s1 = min(B.nSeg, s0 + runLen);
    uint32_t row = carryIn ? carry[t] : PAL_KEY0;                       // after PaletteResetCodeBook every row is (0,0,0)
    for (uint32_t s = s0; s < s1; s++) {
        if (B.segs[s].n == 0) continue;                                 // a skipped pass leaves the book alone
        const uint32_t* book = B.book + (size_t)s * 128;
        if (t < book[0]) row = t ? book[t] : PAL_KEY0;
        B.find[(size_t)s * 64 + t] = row;
    }
    if (carryOut) carry[t] = row;
}

// ---- tokens ------------------------------------------------------------------------------------------------------------------------------------
__device__ inline uint32_t pal_token_bytes(uint32_t b0) { return b0 < 0x80u ? 1u : b0 >= 0xC0u ? 2u : 1u + __popc(b0 & 7u); }

__global__ __launch_bounds__(PAL_WG) void yk_pal_token_kernel(YkPalBufs B) {
    __shared__ uint32_t col[PAL_WG + PAL_BACK];
    __shared__ uint32_t hKey[128], hRow[128];
    __shared__ uint32_t bytes;
    const uint32_t t = threadIdx.x, wg = blockIdx.x;
    const uint32_t sg = pal_find_seg<false>(B.segs, B.nSeg, wg);
    const YkPalSeg S = B.segs[sg];
    const uint32_t base = (wg - S.wg0) * PAL_WG, n = base + t;
    pal_stage(col, S.src, S.n, base, t);
    if (t < 128) { hKey[t] = 0; hRow[t] = 0xFFFFFFFFu; }
    if (t == 0) bytes = 0;
    __syncthreads();
    if (t < 64) {                                                       // delta -> LOWEST row holding it (stale rows make duplicates)
        const uint32_t key = B.find[(size_t)sg * 64 + t];
        uint32_t h = pal_hash(key) >> 25;
        for (;;) {
            const uint32_t old = atomicCAS(&hKey[h], 0u, key);
            if (old == 0u || old == key) { atomicMin(&hRow[h], t); break; }
            h = (h + 1) & 127u;
        }
    }
    __syncthreads();
    auto lookup = [&](uint32_t key) -> uint32_t {                       // 64 rows at most in 128 slots: an empty slot ends every probe
        uint32_t h = pal_hash(key) >> 25;
        for (;;) {
            const uint32_t k = hKey[h];
            if (k == key) return hRow[h];
            if (k == 0u) return 0xFFFFFFFFu;
            h = (h + 1) & 127u;
        }
    };
    if (n >= 1 && n < S.n) {
        const uint32_t me = col[t + PAL_BACK], p1 = col[t + PAL_BACK - 1];
        uint32_t tokv;
        const uint32_t idx0 = lookup(pal_delta_key(me, p1));
        if (idx0 != 0xFFFFFFFFu) tokv = idx0 & 0x7Fu;                   // hit at prev = n - 1: one byte, the walk ends
        else {
            uint32_t best = 0xFFFFFFFFu;                                // row << 7 | j: lowest row, then the nearest prev
            const uint32_t jmax = min(64u, n - 1);
            for (uint32_t j = 1; j <= jmax; j++) {                      // prev = n - 1 - j
                const uint32_t idx = lookup(pal_delta_key(me, col[t + PAL_BACK - 1 - j]));
                if (idx != 0xFFFFFFFFu) best = min(best, (idx << 7) | j);
            }
            if (best != 0xFFFFFFFFu) tokv = (0xC0u | (((best & 127u) - 1u) & 0x3Fu)) | (((best >> 7) & 0x7Fu) << 8);
            else {
                const uint32_t c3[3] = { me & 255u, (me >> 8) & 255u, (me >> 16) & 255u };
                const int d3[3] = { (int)c3[0] - (int)(p1 & 255u), (int)c3[1] - (int)((p1 >> 8) & 255u), (int)c3[2] - (int)((p1 >> 16) & 255u) };
                const bool fits = d3[0] >= -128 && d3[0] <= 127 && d3[1] >= -128 && d3[1] <= 127 && d3[2] >= -128 && d3[2] <= 127;
                tokv = (fits ? 0x80u : 0x88u) | (d3[0] ? 1u : 0u) | (d3[1] ? 2u : 0u) | (d3[2] ? 4u : 0u);
                uint32_t sh = 8;
                for (int k = 0; k < 3; k++) if (d3[k]) { tokv |= (fits ? ((uint32_t)d3[k] & 255u) : c3[k]) << sh; sh += 8; }
            }
        }
        B.tok[S.colOff + n] = tokv;
        atomicAdd(&bytes, pal_token_bytes(tokv & 255u));
    }
    __syncthreads();
    if (t == 0) B.wgBytes[wg] = bytes;
}

// ---- offsets -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PAL_WG) void yk_pal_scan_kernel(YkPalBufs B) {
    __shared__ uint32_t sh[PAL_WG];
    const uint32_t t = threadIdx.x, sg = blockIdx.x;
    const YkPalSeg S = B.segs[sg];
    if (S.n == 0) { if (t == 0) B.segLen[sg] = 0; return; }
    const uint32_t nWg = (S.n + PAL_WG - 1) / PAL_WG;
    uint32_t running = 1u + 3u * min(B.book[(size_t)sg * 128], 128u) + 3u;          // finalCount, its rows, the first colour
    for (uint32_t w0 = 0; w0 < nWg; w0 += PAL_WG) {
        const uint32_t w = w0 + t;
        uint32_t total;
        const uint32_t ex = pal_block_excl(w < nWg ? B.wgBytes[S.wg0 + w] : 0u, sh, t, &total);
        if (w < nWg) B.wgOff[S.wg0 + w] = running + ex;
        running += total;
    }
    if (t == 0) B.segLen[sg] = running;
}

__global__ __launch_bounds__(PAL_WG) void yk_pal_layout_kernel(YkPalBufs B) {
    __shared__ uint32_t sh[PAL_WG];
    const uint32_t t = threadIdx.x;
    uint32_t running = 0;
    for (uint32_t s0 = 0; s0 < B.nSeg; s0 += PAL_WG) {
        const uint32_t s = s0 + t;
        uint32_t total;
        const uint32_t ex = pal_block_excl(s < B.nSeg ? (B.segLen[s] + 15u) & ~15u : 0u, sh, t, &total);
        if (s < B.nSeg) B.segBase[s] = running + ex;
        running += total;
    }
}

// ---- emit --------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PAL_WG) void yk_pal_emit_kernel(YkPalBufs B, uint8_t* __restrict__ out) {
    __shared__ uint32_t sh[PAL_WG];
    const uint32_t t = threadIdx.x, wg = blockIdx.x;
    const uint32_t sg = pal_find_seg<false>(B.segs, B.nSeg, wg);
    const YkPalSeg S = B.segs[sg];
    const uint32_t base = (wg - S.wg0) * PAL_WG, n = base + t;
    uint8_t* dst = out + B.segBase[sg];
    uint32_t tokv = 0, cnt = 0;
    if (n >= 1 && n < S.n) { tokv = B.tok[S.colOff + n]; cnt = pal_token_bytes(tokv & 255u); }
    uint32_t total;
    const uint32_t ex = pal_block_excl(cnt, sh, t, &total);
    uint8_t* q = dst + B.wgOff[wg] + ex;
    for (uint32_t k = 0; k < cnt; k++) q[k] = (uint8_t)(tokv >> (8 * k));
    if (base == 0) {                                                    // the segment's first workgroup also writes the header
        const uint32_t* book = B.book + (size_t)sg * 128;
        const uint32_t finalCount = min(book[0], 128u);
        if (t == 0) dst[0] = (uint8_t)finalCount;
        if (t < finalCount) {
            const uint32_t key = t ? book[t] : PAL_KEY0;
            dst[1 + 3 * t] = (uint8_t)((key & 1023u) - 256u); dst[2 + 3 * t] = (uint8_t)(((key >> 10) & 1023u) - 256u); dst[3 + 3 * t] = (uint8_t)(((key >> 20) & 1023u) - 256u);
        }
        if (t < 3) dst[1 + 3 * finalCount + t] = S.src[t];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
// the caller has validated: 1 <= nSeg <= PAL_MAX_SEGS, every length a multiple of 3, a pointer for every non-empty stream, chain >= 0
static int yk_pal_run(yk_ctx* c, const uint8_t* const* dev, const size_t* nBytes, int nSeg, int chain) {
    YkPalette& P = c->pal;
    size_t colours = 0;
    for (int s = 0; s < nSeg; s++) colours += nBytes[s] / 3;
    if (colours > PAL_MAX_COLOURS) return yk_refuse(c, YK_ERR_BAD_ARG, "more than 2^28 colours in one call");
    YK_HIP(c, hipSetDevice(c->device));
    P.valid = false;
    // ---- the segment table and the carve-up of the scratch buffer ----
    P.segHost.resize((size_t)nSeg * sizeof(YkPalSeg));
    YkPalSeg* segs = reinterpret_cast<YkPalSeg*>(P.segHost.data());
    uint32_t nWg = 0, nSlots = 0, nSlices = 0, nCol = 0, outNeed = 0;
    for (int s = 0; s < nSeg; s++) {
        const uint32_t n = (uint32_t)(nBytes[s] / 3);
        segs[s] = YkPalSeg{ n ? dev[s] : nullptr, n, nWg, nSlots, 0u, nSlices, nCol };
        if (!n) continue;
        segs[s].tabCap = n + n / 2 + 64;                                // every colour may vote for a delta of its own
        nWg += (n + PAL_WG - 1) / PAL_WG; nSlots += segs[s].tabCap; nSlices += (segs[s].tabCap + PAL_SLICE - 1) / PAL_SLICE; nCol += n;
        outNeed += (7u * n + 15u) & ~15u;                               // see the head of this file: a payload is at most 7 bytes per colour
    }
    size_t cur = 0;
    auto place = [&](size_t bytes) { const size_t o = cur; cur = (cur + bytes + 255) & ~(size_t)255; return o; };
    const size_t oSeg = place((size_t)nSeg * sizeof(YkPalSeg));
    const size_t oKey = place((size_t)nSlots * 8), oFirst = place((size_t)nSlots * 4);      // keys and votes together: one clear
    const size_t oCK = place((size_t)nSlices * 128 * 8), oCD = place((size_t)nSlices * 128 * 4), oSC = place((size_t)nSlices * 4);
    const size_t oBook = place((size_t)nSeg * 128 * 4), oFind = place((size_t)nSeg * 64 * 4);
    const size_t oTok = place((size_t)nCol * 4), oWB = place((size_t)nWg * 4), oWO = place((size_t)nWg * 4), oLen = place((size_t)nSeg * 8);
    YK_HIP(c, P.scratch.reserve(c->stream, cur));
    YK_HIP(c, P.out.reserve(c->stream, (size_t)outNeed + 16));
    if (!P.carry) YK_HIP(c, P.carry.alloc(c->stream, 64));
    YkPalBufs B;
    B.segs = reinterpret_cast<const YkPalSeg*>(P.scratch + oSeg); B.nSeg = (uint32_t)nSeg;
    B.tKey = reinterpret_cast<uint32_t*>(P.scratch + oKey); B.tVotes = B.tKey + nSlots; B.tFirst = reinterpret_cast<uint32_t*>(P.scratch + oFirst);
    B.candKey = reinterpret_cast<unsigned long long*>(P.scratch + oCK); B.candDelta = reinterpret_cast<uint32_t*>(P.scratch + oCD);
    B.sliceCnt = reinterpret_cast<uint32_t*>(P.scratch + oSC);
    B.book = reinterpret_cast<uint32_t*>(P.scratch + oBook); B.find = reinterpret_cast<uint32_t*>(P.scratch + oFind);
    B.tok = reinterpret_cast<uint32_t*>(P.scratch + oTok); B.wgBytes = reinterpret_cast<uint32_t*>(P.scratch + oWB); B.wgOff = reinterpret_cast<uint32_t*>(P.scratch + oWO);
    B.segLen = reinterpret_cast<uint32_t*>(P.scratch + oLen); B.segBase = B.segLen + nSeg;
    YK_HIP(c, hipMemcpyAsync(P.scratch + oSeg, segs, (size_t)nSeg * sizeof(YkPalSeg), hipMemcpyHostToDevice, c->stream));
    // ---- the launches ----
    const bool continues = chain == 0;                                  // one run over the handle's carried rows
    const uint32_t runLen = continues ? (uint32_t)nSeg : (uint32_t)chain, nRuns = ((uint32_t)nSeg + runLen - 1) / runLen;
    { int rc = yk_stage_begin(c, YK_STAGE_PALETTE); if (rc) return rc; }
    if (nWg) {
        YK_HIP(c, hipMemsetAsync(B.tKey, 0, (size_t)nSlots * 8, c->stream));
        YK_HIP(c, hipMemsetAsync(B.tFirst, 0xFF, (size_t)nSlots * 4, c->stream));
        hipLaunchKernelGGL(yk_pal_vote_kernel, dim3(nWg), dim3(PAL_WG), 0, c->stream, B);
        hipLaunchKernelGGL(yk_pal_select1_kernel, dim3(nSlices), dim3(PAL_WG), 0, c->stream, B);
    }
    hipLaunchKernelGGL(yk_pal_select2_kernel, dim3((unsigned)nSeg), dim3(PAL_WG), 0, c->stream, B);
    hipLaunchKernelGGL(yk_pal_chain_kernel, dim3(nRuns), dim3(64), 0, c->stream, B, runLen, P.carry, continues && !P.carryFresh ? 1 : 0, continues ? 1 : 0);
    if (nWg) hipLaunchKernelGGL(yk_pal_token_kernel, dim3(nWg), dim3(PAL_WG), 0, c->stream, B);
    hipLaunchKernelGGL(yk_pal_scan_kernel, dim3((unsigned)nSeg), dim3(PAL_WG), 0, c->stream, B);
    hipLaunchKernelGGL(yk_pal_layout_kernel, dim3(1), dim3(PAL_WG), 0, c->stream, B);
    if (nWg) hipLaunchKernelGGL(yk_pal_emit_kernel, dim3(nWg), dim3(PAL_WG), 0, c->stream, B, P.out);
    YK_HIP(c, hipGetLastError());
    { int rc = yk_stage_end(c, YK_STAGE_PALETTE); if (rc) return rc; }
    if (continues) P.carryFresh = false;
    // ---- the one read-back: length and offset of every payload ----
    P.lenBase.resize((size_t)nSeg * 2);
    YK_HIP(c, hipMemcpyAsync(P.lenBase.data(), B.segLen, (size_t)nSeg * 8, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    P.nSeg = nSeg; P.valid = true;
    return YK_OK;
}

extern "C" {

int yk_palette_reset(yk_ctx* c) {
    if (!c) return YK_ERR_BAD_ARG;
    c->pal.carryFresh = true;                                           // the next continuing call starts from 64 rows of (0,0,0)
    return YK_OK;
}

int yk_palette_compress_streams(yk_ctx* c, const uint8_t* const* devStreams, const size_t* nBytes, int nStreams, int chain) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!devStreams || !nBytes) return yk_refuse(c, YK_ERR_BAD_ARG, "devStreams or nBytes is NULL");
    if (nStreams < 1 || nStreams > PAL_MAX_SEGS) return yk_refuse(c, YK_ERR_BAD_ARG, "nStreams must be 1..65536");
    if (chain < 0) return yk_refuse(c, YK_ERR_BAD_ARG, "chain must be 0 (continue the carried book) or the run length K > 0");
    for (int s = 0; s < nStreams; s++) {
        if (nBytes[s] % 3) return yk_refuse(c, YK_ERR_BAD_ARG, "a stream length is not a multiple of 3 (plane-subset streams stay on the host coder)");
        if (nBytes[s] && !devStreams[s]) return yk_refuse(c, YK_ERR_BAD_ARG, "a stream has a length and a NULL pointer");
    }
    return yk_pal_run(c, devStreams, nBytes, nStreams, chain);
}

int yk_palette_compress(yk_ctx* c) {
    if (!c) return YK_ERR_BAD_ARG;
    if (c->y0 != 0 || c->h != c->fullH) return yk_refuse(c, YK_ERR_STATE, "yk_palette_compress works on whole images, not on a stripe");
    if (!c->encoded) return yk_refuse(c, YK_ERR_STATE, "yk_encode_tiles first (or yk_encode_frame / yk_encode_batch)");
    if (c->ppActive) return yk_refuse(c, YK_ERR_STATE, "a plane-subset pass ran: its streams stay on the host coder");
    const uint8_t* dev[7]; size_t nb[7];
    for (int p = 0; p < 7; p++) { int rc = yk_gradient_corners_device(c, p, &dev[p], &nb[p]); if (rc) return rc; }
    return yk_pal_run(c, dev, nb, 7, 0);
}

int yk_palette_compress_batch(yk_ctx* c) {
    if (!c) return YK_ERR_BAD_ARG;
    const YkStreamsBatch& b = c->img.sb;
    if (!b.valid || (int)b.table.size() != c->nFrames || !(b.what & YK_STREAMS_CORNERS))
        return yk_refuse(c, YK_ERR_STATE, "yk_encode_streams_batch with YK_STREAMS_CORNERS first (the table does not outlive an encode, a new image or new planes)");
    const int N = c->nFrames;
    std::vector<const uint8_t*> dev((size_t)N * 7); std::vector<size_t> nb((size_t)N * 7);
    for (int f = 0; f < N; f++) for (int p = 0; p < 7; p++) { dev[(size_t)f * 7 + p] = b.table[(size_t)f].rgb[p]; nb[(size_t)f * 7 + p] = b.table[(size_t)f].rgbBytes[p]; }
    return yk_pal_run(c, dev.data(), nb.data(), N * 7, 7);
}

int yk_palette_payload_device(yk_ctx* c, int index, const uint8_t** dev, size_t* nBytes) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!dev || !nBytes) return yk_refuse(c, YK_ERR_BAD_ARG, "dev or nBytes is NULL");
    if (!c->pal.valid) return yk_refuse(c, YK_ERR_STATE, "yk_palette_compress, yk_palette_compress_batch or yk_palette_compress_streams first (the payloads do not outlive an encode, a new image or new planes)");
    if (index < 0 || index >= c->pal.nSeg) return yk_refuse(c, YK_ERR_BAD_ARG, "payload index out of range");
    const size_t n = c->pal.lenBase[(size_t)index];
    *dev = n ? c->pal.out + c->pal.lenBase[(size_t)c->pal.nSeg + index] : nullptr; *nBytes = n;
    return YK_OK;
}

int yk_palette_payload(yk_ctx* c, int index, uint8_t* hostOut, size_t cap, size_t* nBytes) {
    if (!c) return YK_ERR_BAD_ARG;
    const uint8_t* dev = nullptr; size_t n = 0;
    { int rc = yk_palette_payload_device(c, index, &dev, &n); if (rc) return rc; }
    if (nBytes) *nBytes = n;
    if (!hostOut) return YK_OK;                                         // size query
    if (cap < n) return yk_refuse(c, YK_ERR_RANGE, "payload buffer too small");
    if (n) {
        YK_HIP(c, hipSetDevice(c->device));
        YK_HIP(c, hipMemcpyAsync(hostOut, dev, n, hipMemcpyDeviceToHost, c->stream));
        YK_HIP(c, hipStreamSynchronize(c->stream));
    }
    return YK_OK;
}

}  // extern "C"
