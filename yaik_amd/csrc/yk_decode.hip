// yk_decode.hip — gfx950 kernels for the per-tile decode loops behind YAIK_DecodeImage's chunk switch
// (decoder/YAIK_API.cpp:731-1303):
//
//   yk_decode_gradient   a16  DecompressGradient16x16/16x8/8x16/8x8/8x4/4x8/4x4   (decoder/YAIK_Gradient.cpp:28..1418)
//   yk_decode_1d         a17  Decompress1D x 3 planes                              (decoder/YAIK_3DTile.cpp:24-240)
//   yk_decode_mask       a18  Decompress1BitTiled                                  (decoder/YAIK_Mipmap.cpp:23-154)
//
// HBM layout mirrors YAIK_Instance (include/YAIK_private.h:26-54): planeR|G|B u8 in 8x8 tiles (tile-major, 64 B/tile,
// include/YAIK.h:205-224), the mapRGB corner lattice ((W/4+1) x (H/4+1) x 3 u8) and tile4x4Mask (1 bit per 4x4 cell).
// The reference walks each bitmap sequentially and pops "not yet seen" corners off the colour stream; on the GPU the
// stream offset of every tile is a prefix sum over the bitmap words of the corners each tile is the FIRST to touch
// (first toucher by scan position = atomicMin of bitIndex<<2|corner), then all tiles of the pass render in parallel.
// Passes are launched in call order, so a later, overlapping tile overwrites an earlier one exactly like the reference.
#include "yk_common.h"
#include "yk_device.h"
#include "yk_window_blocks.h"
#include "yk_window_px.h"
#include "yk_window_mirror.h"
#include "yk_resample.h"

struct DPassGeo { int sx, sy, bigX, bigY, bitCount, xBB, tilesPerRow; };

__host__ __device__ static inline DPassGeo yk_dpass_geo(int sx, int sy, int w) {
    DPassGeo g; g.sx = sx; g.sy = sy;
    g.bigX = sx == 2 ? 32 : 64; g.bigY = sy == 2 ? 32 : 64;            // getSwizzleSize, include/YAIK_private.h:212-276
    g.tilesPerRow = g.bigX >> sx; g.bitCount = g.tilesPerRow * (g.bigY >> sy);
    g.xBB = (w + g.bigX - 1) / g.bigX;
    return g;
}

__device__ __forceinline__ void yk_dtile_from_bit(const DPassGeo& g, uint32_t pos, int& x, int& y) {
    const uint32_t blk = pos / g.bitCount, t = pos % g.bitCount;
    x = (int)(blk % g.xBB) * g.bigX + (int)(t % g.tilesPerRow) * (1 << g.sx);
    y = (int)(blk / g.xBB) * g.bigY + (int)(t / g.tilesPerRow) * (1 << g.sy);
}

// phase 1: first toucher of every not-yet-loaded lattice point.  One thread per tile slot (bit) of the bitmap.
__global__ __launch_bounds__(256) void yk_dec_owner_kernel(const uint32_t* __restrict__ bitmap, size_t nBits, DPassGeo g, int w, int h, int latW,
                                                           const uint8_t* __restrict__ loaded, uint32_t* __restrict__ owner) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= nBits || !((bitmap[pos >> 5] >> (pos & 31)) & 1u)) return;
    const int dx = 1 << (g.sx - 2), dy = 1 << (g.sy - 2);
    int x, y; yk_dtile_from_bit(g, (uint32_t)pos, x, y);
    if (x + (1 << g.sx) > w || y + (1 << g.sy) > h) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t li = (size_t)((y >> 2) + ((k & 2) ? dy : 0)) * latW + (x >> 2) + ((k & 1) ? dx : 0);
        if (!(loaded[li] & 1)) atomicMin(&owner[li], ((uint32_t)pos << 2) | (uint32_t)k);      // mapRGBMask plane 0 (hasRGB)
    }
}

// phase 2 (EMIT=false): corners owned per workgroup of 1024 tile slots; phase 3 (EMIT=true): pop the colours into the
// lattice (:97-136) at the offsets an exclusive scan over the owned-corner counts gives.
template <bool EMIT>
__global__ __launch_bounds__(1024) void yk_dec_corner_kernel(const uint32_t* __restrict__ bitmap, size_t nBits, DPassGeo g, int w, int h, int latW,
                                                             uint8_t* __restrict__ loaded, const uint32_t* __restrict__ owner, uint32_t* __restrict__ blockSums,
                                                             const uint8_t* __restrict__ rgb, size_t rgbBytes, uint8_t* __restrict__ mapRGB) {
    __shared__ uint32_t s_tmp[32];
    const size_t pos = (size_t)blockIdx.x * 1024 + threadIdx.x;
    const int dx = 1 << (g.sx - 2), dy = 1 << (g.sy - 2);
    bool set = pos < nBits && ((bitmap[pos >> 5] >> (pos & 31)) & 1u);
    int x = 0, y = 0;
    if (set) { yk_dtile_from_bit(g, (uint32_t)pos, x, y); set = !(x + (1 << g.sx) > w || y + (1 << g.sy) > h); }
    uint32_t own = 0;
    size_t li[4] = { 0, 0, 0, 0 };
    if (set) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            li[k] = (size_t)((y >> 2) + ((k & 2) ? dy : 0)) * latW + (x >> 2) + ((k & 1) ? dx : 0);
            own |= (owner[li[k]] == (((uint32_t)pos << 2) | (uint32_t)k)) ? (1u << k) : 0u;
        }
    }
    uint32_t tot;
    const uint32_t ex = yk_block_exscan((uint32_t)__popc(own), s_tmp, &tot);
    if (!EMIT) { if (threadIdx.x == 0) blockSums[blockIdx.x] = tot; return; }
    uint32_t off = (blockSums[blockIdx.x] + ex) * 3u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!((own >> k) & 1u)) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) mapRGB[li[k] * 3 + c] = (off + c < rgbBytes) ? rgb[off + c] : 0;
        loaded[li[k]] |= 1;
        off += 3;
    }
}

// phase 4: integer bilinear fill with truncation (:160-188, :762-781, :1382-1401) + tile4x4Mask marking.
// One workgroup per bitmap word.  The word's tiles are listed in LDS and the (tile, channel, row, run) items are spread over all 256
// threads, so small tiles keep the workgroup as busy as large ones.  A thread produces a run of min(TX, 8) pixels of one row
// and channel: in the 8x8-tiled plane layout that run is contiguous and leaves as ONE 8-byte (or 4-byte) store.
template <int NW> struct DRenderLdsN { int xy[32 * NW][2]; uint8_t c[32 * NW][3][4]; };
typedef DRenderLdsN<1> DRenderLds;
// A decode window (yk_decode_set_window) rounded out to 64-pixel blocks and clipped to the image: [x0, x1) x [y0, y1) in pixels.  Every tile
// shape's swizzle blocks are 32 or 64 pixels wide and high, so a gradient tile lies inside this rectangle or outside it, never across its border.
struct DWinRect { int x0, y0, x1, y1; };
// WIN of yk_dec_render_words: the whole-image form; every tile of the words lies outside the window (marks only: the tile list and the atomicOr
// marks, no lattice fetch and no plane store); the tiles are tested one by one against the rectangle (a 16x16 word holds two 64x64 blocks)
enum { YK_DR_WHOLE = 0, YK_DR_MARKS = 1, YK_DR_PER_TILE = 2 };
#define YK_DR_SKIP 0x40000000                               // in L.xy[k][1] (YK_DR_PER_TILE): the tile lies outside the window
// the tiles of NW bitmap words (word k: index wi[k], bits bits[k]) of one pass, rendered together by the whole workgroup (256 threads)
template <int NW, int WIN = YK_DR_WHOLE>
__device__ __forceinline__ void yk_dec_render_words(DRenderLdsN<NW>& L, const uint32_t* wi, const uint32_t* bitsN, const DPassGeo& g, int w, int h, int latW,
                                                    const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes, size_t planeSize, int tileW,
                                                    uint32_t* __restrict__ tile4, int stride4, const DWinRect wr = DWinRect{ 0, 0, 0, 0 }) {
    const int TX = 1 << g.sx, TY = 1 << g.sy, dx = TX >> 2, dy = TY >> 2;
    const int lgGpr = g.sx > 3 ? g.sx - 3 : 0, lgPer = g.sy + lgGpr;            // runs per row, runs per channel (powers of two)
    const int GW = TX < 8 ? TX : 8, gpr = 1 << lgGpr, perCh = 1 << lgPer, nEl = 3 * perCh, sh = g.sx + g.sy;
    int nT = 0;
    {
        const int wk = threadIdx.x >> 5, bit = threadIdx.x & 31;
        int before = 0;
#pragma unroll
        for (int k = 0; k < NW; k++) { const int pc = __popc(bitsN[k]); before += (k < wk) ? pc : 0; nT += pc; }
        if (wk < NW && ((bitsN[wk] >> bit) & 1u)) {
            int x, y; yk_dtile_from_bit(g, wi[wk] * 32u + (uint32_t)bit, x, y);
            const int k = before + __popc(bitsN[wk] & ((1u << bit) - 1u));
            L.xy[k][0] = (x + TX > w || y + TY > h) ? -1 : x;
            if (WIN == YK_DR_PER_TILE && (x < wr.x0 || x >= wr.x1 || y < wr.y0 || y >= wr.y1)) y |= YK_DR_SKIP;
            L.xy[k][1] = y;
        }
    }
    __syncthreads();
    if (WIN != YK_DR_MARKS) {                                                   // fetch and fill (kept at its indentation): not for marks only
    // the four corner colours of the word's tiles, once (every run of a tile used to fetch them again: 4 byte loads per 8-byte store)
    // one (unaligned) 4-byte load per corner = its three colours (the lattice array is allocated four bytes longer), not three byte loads
    for (int i = threadIdx.x; i < nT * 4; i += 256) {
        const int k = i >> 2, q = i & 3;
        const int x = L.xy[k][0], y = L.xy[k][1];
        if (x < 0 || (WIN == YK_DR_PER_TILE && (y & YK_DR_SKIP))) continue;
        const size_t li = (size_t)((y >> 2) + ((q & 2) ? dy : 0)) * latW + (x >> 2) + ((q & 1) ? dx : 0);
        uint32_t rgb; __builtin_memcpy(&rgb, mapRGB + li * 3, 4);
        L.c[k][0][q] = (uint8_t)rgb; L.c[k][1][q] = (uint8_t)(rgb >> 8); L.c[k][2][q] = (uint8_t)(rgb >> 16);
    }
    __syncthreads();
    for (int item = threadIdx.x; item < nT * nEl; item += 256) {
        const int ck = item >> lgPer, k = ck / 3, c = ck - 3 * k;           // tile of the list, channel
        const int x = L.xy[k][0], y = L.xy[k][1];
        if (x < 0 || (WIN == YK_DR_PER_TILE && (y & YK_DR_SKIP))) continue;
        const int r = item & (perCh - 1), ty = r >> lgGpr, gx = (r & (gpr - 1)) * GW;
        const uint32_t c4 = *reinterpret_cast<const uint32_t*>(&L.c[k][c][0]);
        const int TL = c4 & 255, TR = (c4 >> 8) & 255, BL = (c4 >> 16) & 255, BR = c4 >> 24;
        const int Lf = TL * (TY - ty) + BL * ty, R = TR * (TY - ty) + BR * ty;
        int v = Lf * (TX - gx) + R * gx;                                    // numerator at the first pixel of the run, + (R - L) per pixel
        const int xx = x + gx, yy = y + ty;
        uint8_t* o = planes + (size_t)c * planeSize + ((size_t)(yy >> 3) * tileW + (xx >> 3)) * 64 + (yy & 7) * 8 + (xx & 7);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) { lo |= (uint32_t)((v >> sh) & 255) << (8 * i); v += R - Lf; }
        if (GW == 8) {
#pragma unroll
            for (int i = 0; i < 4; i++) { hi |= (uint32_t)((v >> sh) & 255) << (8 * i); v += R - Lf; }
            *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
        } else *reinterpret_cast<uint32_t*>(o) = lo;
    }
    }                                                                           // WIN != YK_DR_MARKS
    // cell (cx,cy) -> byte (cx>>2) + (cy>>1)*stride4, bit ((cx>>1)&1)*4 + (cy&1)*2 + (cx&1)   (e.g. YAIK_Gradient.cpp:951-953).  A tile's
    // cells lie in at most two mask bytes (one per pair of cell rows; tiles are at most 4 cells wide and aligned to their size): one
    // atomic per byte with all of the tile's bits in it (one per CELL was 16 device-scope atomics per 16x16 tile: most of this kernel)
    for (int item = threadIdx.x; item < nT * 2; item += 256) {
        const int k = item >> 1, j = item & 1;
        const int x = L.xy[k][0], y = WIN == YK_DR_PER_TILE ? L.xy[k][1] & ~YK_DR_SKIP : L.xy[k][1];
        if (x < 0) continue;
        const int cx0 = x >> 2, cy0 = y >> 2, br = (cy0 >> 1) + j;                // byte row
        if (br > ((cy0 + dy - 1) >> 1)) continue;
        uint32_t m = 0;
        for (int cy = max(cy0, br * 2); cy < min(cy0 + dy, br * 2 + 2); cy++)
            for (int cx = cx0; cx < cx0 + dx; cx++) m |= 1u << ((((cx >> 1) & 1) << 2) | ((cy & 1) << 1) | (cx & 1));
        const size_t byteIdx = (size_t)(cx0 >> 2) + (size_t)br * stride4;
        atomicOr(&tile4[byteIdx >> 2], m << (8 * (byteIdx & 3)));      // (collecting a 64x64 block's marks in LDS and merging them with eight atomics was slower: 105 against 97 us)
    }
}
__device__ __forceinline__ void yk_dec_render_word(DRenderLds& L, const size_t wi, const uint32_t bits, const DPassGeo& g, int w, int h, int latW,
                                                   const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes, size_t planeSize, int tileW,
                                                   uint32_t* __restrict__ tile4, int stride4) {
    const uint32_t wi1[1] = { (uint32_t)wi }, b1[1] = { bits };
    yk_dec_render_words<1>(L, wi1, b1, g, w, h, latW, mapRGB, planes, planeSize, tileW, tile4, stride4);
}

__global__ __launch_bounds__(256) void yk_dec_render_kernel(const uint32_t* __restrict__ bitmap, size_t nWords, DPassGeo g, int w, int h, int latW,
                                                            const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes, size_t planeSize, int tileW,
                                                            uint32_t* __restrict__ tile4, int stride4) {
    __shared__ DRenderLds L;
    const size_t wi = blockIdx.x;
    const uint32_t bits = bitmap[wi];
    if (!bits) return;
    yk_dec_render_word(L, wi, bits, g, w, h, latW, mapRGB, planes, planeSize, tileW, tile4, stride4);
}

// the same under a decode window: tiles outside the window's 64-blocks are marked, not rendered
__global__ __launch_bounds__(256) void yk_dec_render_win_kernel(const uint32_t* __restrict__ bitmap, size_t nWords, DPassGeo g, int w, int h, int latW,
                                                                const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes, size_t planeSize, int tileW,
                                                                uint32_t* __restrict__ tile4, int stride4, const DWinRect wr) {
    __shared__ DRenderLds L;
    const uint32_t wi1[1] = { blockIdx.x }, b1[1] = { bitmap[blockIdx.x] };
    if (!b1[0]) return;
    yk_dec_render_words<1, YK_DR_PER_TILE>(L, wi1, b1, g, w, h, latW, mapRGB, planes, planeSize, tileW, tile4, stride4, wr);
}

// ---- all gradient chunks of a file in one call (yk_decode_gradient_all_device): the passes share every launch ---------------------------------
// What the per-pass sequence above does pass after pass (first toucher among the lattice points no EARLIER pass loaded, count, scan, pop the
// colours) is one first-toucher problem over all passes when the key carries the pass: owner = min(pass << 27 | bitIndex << 2 | corner), the
// layout of yk_corners.hip on the encoder side.  Bitmap bytes (8 tile slots) of all passes are laid end to end; 1024 bytes per workgroup.
struct DecPlan {
    uint32_t byteStart[8], blockStart[8];                   // first bitmap byte / 1024-byte block of pass p ([n..7] = totals)
    uint32_t nBytes[7], rgbBytes[7];
    const uint8_t* bm[7];
    const uint8_t* rgb[7];
    int sx[7], sy[7];
    int n;
};
__device__ __forceinline__ int yk_dplan_find(const uint32_t (&start)[8], uint32_t i) {
    int p = 0;
#pragma unroll
    for (int k = 1; k < 7; k++) p += (i >= start[k]) ? 1 : 0;
    return p;
}
// tiles of a bitmap byte: the 8 slots lie in one swizzle block (every block holds a multiple of 8 tiles); tiles per row / block are powers of two
struct DByteGeo { int bx0, by0, tprShift, tprMask; uint32_t t0; };
__device__ __forceinline__ DByteGeo yk_dbyte_geo(const DPassGeo& g, uint32_t bi) {
    DByteGeo b;
    const uint32_t pos0 = bi * 8u, blk = pos0 / (uint32_t)g.bitCount;
    b.t0 = pos0 % (uint32_t)g.bitCount;
    b.bx0 = (int)(blk % (uint32_t)g.xBB) * g.bigX; b.by0 = (int)(blk / (uint32_t)g.xBB) * g.bigY;
    b.tprShift = __ffs(g.tilesPerRow) - 1; b.tprMask = g.tilesPerRow - 1;
    return b;
}

// The bodies of the all-passes kernels are __device__ functions: the single-image kernels call them with the plan in their arguments and the image's
// arrays, the batch kernels (yk_*_batch_kernel below) with frame blockIdx.y's plan from the table in HBM and that frame's arrays.  blk = blockIdx.x.
__device__ __forceinline__ void yk_decall_owner_body(const DecPlan& pl, int w, int h, int latW, const uint8_t* __restrict__ loaded, uint32_t* __restrict__ owner, const uint32_t blk) {
    const uint32_t gi = blk * blockDim.x + threadIdx.x;
    if (gi >= pl.byteStart[7]) return;
    const int pass = yk_dplan_find(pl.byteStart, gi);
    const uint32_t bi = gi - pl.byteStart[pass];
    const uint32_t byte = pl.bm[pass][bi];
    if (!byte) return;
    const DPassGeo g = yk_dpass_geo(pl.sx[pass], pl.sy[pass], w);
    const DByteGeo b = yk_dbyte_geo(g, bi);
    const int dx = 1 << (g.sx - 2), dy = 1 << (g.sy - 2);
    // tiles of the byte that lie inside the image (the reference skips the others, :58-60)
    uint32_t live = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t t = b.t0 + (uint32_t)k;
        const int x = b.bx0 + (int)((t & (uint32_t)b.tprMask) << g.sx), y = b.by0 + (int)((t >> b.tprShift) << g.sy);
        if (((byte >> k) & 1u) && !(x + (1 << g.sx) > w || y + (1 << g.sy) > h)) live |= 1u << k;
    }
    const bool two = g.tilesPerRow == 4;                                     // the byte is one row of 8 tiles, or two rows of 4
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (!((live >> k) & 1u)) continue;
        const uint32_t t = b.t0 + (uint32_t)k;
        const int x = b.bx0 + (int)((t & (uint32_t)b.tprMask) << g.sx), y = b.by0 + (int)((t >> b.tprShift) << g.sy);
        const uint32_t key = ((uint32_t)pass << 27) | ((bi * 8u + (uint32_t)k) << 2);
        // a corner an EARLIER live tile of this same byte also touches belongs to that tile (smaller scan position): no atomic for it
        // (left, upper, upper-left, upper-right neighbours; yk_corners.hip measured 32 -> 15 atomics for a dense group of 16x16 tiles)
        const int col = (int)(t & (uint32_t)b.tprMask);
        const bool left = k >= 1 && col != 0 && ((live >> (k - 1)) & 1u);
        const bool up = two && k >= 4 && ((live >> (k - 4)) & 1u);
        const bool upLeft = two && k >= 5 && col != 0 && ((live >> (k - 5)) & 1u);
        const bool upRight = two && k >= 4 && col != 3 && ((live >> (k - 3)) & 1u);
        const bool skip[4] = { left || up || upLeft, up || upRight, left, false };
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (skip[q]) continue;
            const size_t li = (size_t)((y >> 2) + ((q & 2) ? dy : 0)) * latW + (x >> 2) + ((q & 1) ? dx : 0);
            if (!(loaded[li] & 1)) atomicMin(&owner[li], key | (uint32_t)q);
        }
    }
}

__global__ __launch_bounds__(256) void yk_decall_owner_kernel(const DecPlan pl, int w, int h, int latW, const uint8_t* __restrict__ loaded, uint32_t* __restrict__ owner) {
    yk_decall_owner_body(pl, w, h, latW, loaded, owner, blockIdx.x);
}

// COUNT: corners owned per thread (4 bits per tile slot, kept for the emit launch) and per workgroup.
// EMIT: the owners pop their colours off the pass's stream (offset = scanned corners before them x 3) into the lattice.
template <bool EMIT>
__device__ __forceinline__ void yk_decall_stream_body(const DecPlan& pl, int w, int h, int latW, uint8_t* __restrict__ loaded, const uint32_t* __restrict__ owner,
                                                      uint32_t* __restrict__ blockSums, uint32_t* __restrict__ perThread, uint8_t* __restrict__ mapRGB, uint32_t factor,
                                                      const uint32_t blk) {
    __shared__ uint32_t s_tmp[32];
    const int pass = yk_dplan_find(pl.blockStart, blk);
    const uint32_t bi = (blk - pl.blockStart[pass]) * 1024u + threadIdx.x;
    const uint32_t nBytes = pl.nBytes[pass];
    const size_t ti = (size_t)pl.byteStart[pass] + bi;
    const uint32_t byte = bi < nBytes ? pl.bm[pass][bi] : 0u;
    const DPassGeo g = yk_dpass_geo(pl.sx[pass], pl.sy[pass], w);
    const int dx = 1 << (g.sx - 2), dy = 1 << (g.sy - 2);
    // COUNT leaves the thread's ownership bits (4 per tile slot) for EMIT, which then neither repeats the 32 owner look-ups nor waits for them
    uint32_t cnt = 0, ownBits = 0;
    if (EMIT) { ownBits = bi < nBytes ? perThread[ti] : 0u; cnt = (uint32_t)__popc(ownBits); }
    uint32_t own[8];
    int tx[8], ty[8];
    if ((!EMIT && byte) || cnt) {
        const DByteGeo b = yk_dbyte_geo(g, bi);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t t = b.t0 + (uint32_t)k;
            tx[k] = b.bx0 + (int)((t & (uint32_t)b.tprMask) << g.sx); ty[k] = b.by0 + (int)((t >> b.tprShift) << g.sy);
        }
        if (EMIT) {
#pragma unroll
            for (int k = 0; k < 8; k++) own[k] = (ownBits >> (4 * k)) & 15u;
        } else {
            uint32_t o[8][4];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const bool set = ((byte >> k) & 1u) && !(tx[k] + (1 << g.sx) > w || ty[k] + (1 << g.sy) > h);
                const size_t l0 = set ? (size_t)(ty[k] >> 2) * latW + (tx[k] >> 2) : 0;
                const size_t ddx = set ? dx : 0, ddy = set ? (size_t)dy * latW : 0;
                o[k][0] = owner[l0]; o[k][1] = owner[l0 + ddx]; o[k][2] = owner[l0 + ddy]; o[k][3] = owner[l0 + ddy + ddx];
                const uint32_t key = ((uint32_t)pass << 27) | ((bi * 8u + (uint32_t)k) << 2);
                own[k] = set ? ((o[k][0] == (key | 0u) ? 1u : 0u) | (o[k][1] == (key | 1u) ? 2u : 0u) | (o[k][2] == (key | 2u) ? 4u : 0u) | (o[k][3] == (key | 3u) ? 8u : 0u)) : 0u;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) { own[k] = 0; tx[k] = 0; ty[k] = 0; }
    }
    if (!EMIT) {
#pragma unroll
        for (int k = 0; k < 8; k++) { cnt += (uint32_t)__popc(own[k]); ownBits |= own[k] << (4 * k); }
        uint32_t tot;
        yk_block_exscan(cnt, s_tmp, &tot);
        if (bi < nBytes) perThread[ti] = ownBits;
        if (threadIdx.x == 0) blockSums[blk] = tot;
        return;
    }
    uint32_t tot;
    const uint32_t ex = yk_block_exscan(cnt, s_tmp, &tot);
    constexpr uint32_t kCap = 8192;                                          // colours listed per workgroup
    __shared__ uint32_t s_li[kCap];
    const uint32_t blockOff = (blockSums[blk] - blockSums[pl.blockStart[pass]]) * 3u;
    const uint8_t* const rgb = pl.rgb[pass];
    const uint32_t rgbBytes = pl.rgbBytes[pass];
    auto colour = [&](const uint32_t li, const uint32_t j) {                 // the j-th colour of the workgroup goes to lattice point li (:97-136)
        const uint32_t off = blockOff + j * 3u;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            uint32_t v = (off + ch < rgbBytes) ? rgb[off + ch] : 0u;
            if (factor) v = (v * factor) >> 16;                              // PaletteFullRangeRemapping (YAIK_GenericFunctions.cpp:128-137)
            mapRGB[(size_t)li * 3 + ch] = (uint8_t)v;
        }
        loaded[li] |= 1;
    };
    const bool viaLds = tot <= kCap;
    if (cnt) {
        uint32_t j = ex;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (!own[k]) continue;
#pragma unroll
            for (int c4 = 0; c4 < 4; c4++) {
                if (!((own[k] >> c4) & 1u)) continue;
                const uint32_t li = (uint32_t)((ty[k] >> 2) + ((c4 & 2) ? dy : 0)) * (uint32_t)latW + (uint32_t)((tx[k] >> 2) + ((c4 & 1) ? dx : 0));
                if (viaLds) s_li[j] = li; else colour(li, j);
                j++;
            }
        }
    }
    if (!viaLds) return;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < tot; j += 1024) colour(s_li[j], j);
}

template <bool EMIT>
__global__ __launch_bounds__(1024) void yk_decall_stream_kernel(const DecPlan pl, int w, int h, int latW, uint8_t* __restrict__ loaded, const uint32_t* __restrict__ owner,
                                                                uint32_t* __restrict__ blockSums, uint32_t* __restrict__ perThread, uint8_t* __restrict__ mapRGB,
                                                                uint32_t factor) {
    yk_decall_stream_body<EMIT>(pl, w, h, latW, loaded, owner, blockSums, perThread, mapRGB, factor, blockIdx.x);
}

// exclusive prefix of the per-block corner counts in place (one workgroup: thread t owns a run of consecutive blocks)
__device__ __forceinline__ void yk_decall_scan_body(uint32_t* __restrict__ blockSums, const DecPlan& pl) {
    __shared__ uint32_t s_tmp[32];
    const uint32_t n = pl.blockStart[7], per = (n + 1023) / 1024;
    const uint32_t a = min(threadIdx.x * per, n), b = min(a + per, n);
    uint32_t sum = 0;
    for (uint32_t i = a; i < b; i++) sum += blockSums[i];
    uint32_t tot;
    uint32_t run = yk_block_exscan(sum, s_tmp, &tot);
    for (uint32_t i = a; i < b; i++) { const uint32_t v = blockSums[i]; blockSums[i] = run; run += v; }
}

__global__ __launch_bounds__(1024) void yk_decall_scan_kernel(uint32_t* __restrict__ blockSums, const DecPlan pl) {
    yk_decall_scan_body(blockSums, pl);
}

// ONE render launch for all passes: a workgroup owns a 64x64 block of the image and walks the passes in call order, rendering the tiles of the
// bitmap words that cover its block (every tile shape's swizzle blocks are 64 or 32 pixels wide and high: at most 20.5 words per block and frame).
// A later, overlapping tile still overwrites an earlier one like the reference (same workgroup, passes in order, stores of a pass acknowledged
// before the next one starts); no lists of non-empty words are needed (an empty block costs its workgroup seven small loads), and seven dependent
// launches of 16 us each (0.11 ms of the 0.33 ms decode of an 8192 x 8192 frame) become one.
// WIN: under a decode window a workgroup whose block lies outside wr (the window in whole 64-blocks) only marks its tiles in tile4x4Mask, which
// the 1-D count reads for every tile of the image; the decision is uniform over the workgroup
template <bool WIN>
__device__ __forceinline__ void yk_decall_render_blocks_body(const DecPlan& pl, int w, int h, int latW, const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes,
                                                             size_t planeSize, int tileW, uint32_t* __restrict__ tile4, int stride4, const uint32_t blk,
                                                             const DWinRect wr = DWinRect{ 0, 0, 0, 0 }) {
    __shared__ DRenderLdsN<8> L;
    __shared__ uint32_t s_word[7][8], s_idx[7][8];
    const int xB64 = (w + 63) >> 6;
    const int bx64 = (int)(blk % (unsigned)xB64), by64 = (int)(blk / (unsigned)xB64);
    // the (up to 8) words of every pass that cover this block, fetched together: thread = pass * 8 + slot
    if (threadIdx.x < 56) {
        const int p = threadIdx.x >> 3, k = threadIdx.x & 7;
        uint32_t bits = 0, wi = 0;
        if (p < pl.n) {
            const DPassGeo g = yk_dpass_geo(pl.sx[p], pl.sy[p], w);
            const int nbx = 64 / g.bigX, nby = 64 / g.bigY, wpb = g.bitCount >= 32 ? g.bitCount >> 5 : 1;      // swizzle blocks per 64x64 block, words per swizzle block
            const int sb = k / wpb, wk = k - sb * wpb;
            if (sb < nbx * nby) {
                const int sbx = bx64 * nbx + (sb % nbx), sby = by64 * nby + (sb / nbx), yBB = (h + g.bigY - 1) / g.bigY;
                if (sbx < g.xBB && sby < yBB) {
                    const uint32_t bit0 = (uint32_t)(sby * g.xBB + sbx) * (uint32_t)g.bitCount;
                    wi = (bit0 >> 5) + (uint32_t)wk;
                    const uint32_t b0 = wi * 4u;
#pragma unroll
                    for (int j = 0; j < 4; j++) if (b0 + j < pl.nBytes[p]) bits |= (uint32_t)pl.bm[p][b0 + j] << (8 * j);
                    if (g.bitCount < 32) bits &= 0xFFFFu << (bit0 & 31u);        // 16x16: two blocks share a word
                }
            }
        }
        s_word[p][k] = bits; s_idx[p][k] = wi;
    }
    __syncthreads();
    if (WIN && (bx64 * 64 < wr.x0 || bx64 * 64 >= wr.x1 || by64 * 64 < wr.y0 || by64 * 64 >= wr.y1)) {
        bool listed = false;
        for (int p = 0; p < pl.n; p++) {
            uint32_t bits8[8], idx8[8], any = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) { bits8[k] = s_word[p][k]; idx8[k] = s_idx[p][k]; any |= bits8[k]; }
            if (!any) continue;
            if (listed) __syncthreads();                                          // the previous pass's tile list has been read
            const DPassGeo g = yk_dpass_geo(pl.sx[p], pl.sy[p], w);
            yk_dec_render_words<8, YK_DR_MARKS>(L, idx8, bits8, g, w, h, latW, mapRGB, planes, planeSize, tileW, tile4, stride4);
            listed = true;
        }
        return;
    }
    bool wrote = false;
    for (int p = 0; p < pl.n; p++) {
        uint32_t bits8[8], idx8[8], any = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) { bits8[k] = s_word[p][k]; idx8[k] = s_idx[p][k]; any |= bits8[k]; }
        if (!any) continue;                                                       // uniform over the workgroup
        if (wrote) { __threadfence_block(); __syncthreads(); }                   // the previous pass's stores are out and its LDS image is free
        const DPassGeo g = yk_dpass_geo(pl.sx[p], pl.sy[p], w);
        yk_dec_render_words<8>(L, idx8, bits8, g, w, h, latW, mapRGB, planes, planeSize, tileW, tile4, stride4);
        wrote = true;
    }
}

__global__ __launch_bounds__(256) void yk_decall_render_blocks_kernel(const DecPlan pl, int w, int h, int latW, const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes,
                                                                      size_t planeSize, int tileW, uint32_t* __restrict__ tile4, int stride4) {
    yk_decall_render_blocks_body<false>(pl, w, h, latW, mapRGB, planes, planeSize, tileW, tile4, stride4, blockIdx.x);
}
__global__ __launch_bounds__(256) void yk_decall_render_blocks_win_kernel(const DecPlan pl, int w, int h, int latW, const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes,
                                                                          size_t planeSize, int tileW, uint32_t* __restrict__ tile4, int stride4, const DWinRect wr) {
    yk_decall_render_blocks_body<true>(pl, w, h, latW, mapRGB, planes, planeSize, tileW, tile4, stride4, blockIdx.x, wr);
}
// a prepared image (yk_decode_prepare_device): the blocks of a list (ascending, each once: two workgroups on one block would break the order of
// the passes inside it).  The marks are issued again; tile4x4Mask holds them already, so it does not change.
__global__ __launch_bounds__(256) void yk_decall_render_blocks_list_kernel(const DecPlan pl, int w, int h, int latW, const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes,
                                                                           size_t planeSize, int tileW, uint32_t* __restrict__ tile4, int stride4, const uint32_t* __restrict__ list) {
    yk_decall_render_blocks_body<false>(pl, w, h, latW, mapRGB, planes, planeSize, tileW, tile4, stride4, list[blockIdx.x]);
}

// ---- the same five launches over a batch: frame = blockIdx.y -------------------------------------------------------------------------------
// Every frame of a batch has the shape of every other, so byteStart / blockStart, the grids and the scratch layout are those of one
// image; the frames differ in their stream pointers and colour-stream lengths.  A DecPlan is 296 bytes: up to 1024 of them do not fit kernel
// arguments, so the call writes them once into a table in HBM and a workgroup reads its frame's plan through scalar loads (uniform address).
// Frame f's arrays lie at base + f * stride (bytes), its scratch arrays at scratch + f * sScratch + the offsets of the single-image call.
struct DecBatch {
    const DecPlan* plans;
    uint8_t* loaded; uint8_t* owner; uint8_t* mapRGB; uint8_t* planes; uint8_t* tile4; uint8_t* scratch;
    size_t sLoaded, sOwner, sMapRGB, sPlanes, sTile4, sScratch;
    size_t oSums, oPerThread;
};
__device__ __forceinline__ uint32_t* yk_dbatch_u32(const DecBatch& B, size_t f, size_t off) { return reinterpret_cast<uint32_t*>(B.scratch + f * B.sScratch + off); }

__global__ __launch_bounds__(256) void yk_decall_owner_batch_kernel(const DecBatch B, int w, int h, int latW) {
    const size_t f = blockIdx.y;
    yk_decall_owner_body(B.plans[f], w, h, latW, B.loaded + f * B.sLoaded, reinterpret_cast<uint32_t*>(B.owner + f * B.sOwner), blockIdx.x);
}
template <bool EMIT>
__global__ __launch_bounds__(1024) void yk_decall_stream_batch_kernel(const DecBatch B, int w, int h, int latW, uint32_t factor) {
    const size_t f = blockIdx.y;
    yk_decall_stream_body<EMIT>(B.plans[f], w, h, latW, B.loaded + f * B.sLoaded, reinterpret_cast<const uint32_t*>(B.owner + f * B.sOwner), yk_dbatch_u32(B, f, B.oSums),
                                yk_dbatch_u32(B, f, B.oPerThread), B.mapRGB + f * B.sMapRGB, factor, blockIdx.x);
}
__global__ __launch_bounds__(1024) void yk_decall_scan_batch_kernel(const DecBatch B) {       // one workgroup per frame
    const size_t f = blockIdx.x;
    yk_decall_scan_body(yk_dbatch_u32(B, f, B.oSums), B.plans[f]);
}
__global__ __launch_bounds__(256) void yk_decall_render_blocks_batch_kernel(const DecBatch B, int w, int h, int latW, size_t planeSize, int tileW, int stride4) {
    const size_t f = blockIdx.y;
    yk_decall_render_blocks_body<false>(B.plans[f], w, h, latW, B.mapRGB + f * B.sMapRGB, B.planes + f * B.sPlanes, planeSize, tileW,
                                 reinterpret_cast<uint32_t*>(B.tile4 + f * B.sTile4), stride4, blockIdx.x);
}
// A batch whose frames have windows (yk_decode_set_batch_windows): frame f's exact rectangle {x0, y0, x1, y1} is entry f of a table in HBM (like the
// plans: up to 1024 of them do not fit kernel arguments), read by every workgroup of the frame through a uniform address
__device__ __forceinline__ DWinRect yk_bwin_rect64(const DWinRect e, int w, int h) {      // ... rounded out to 64-pixel blocks, clipped to the image
    DWinRect r = { e.x0 & ~63, e.y0 & ~63, (e.x1 + 63) & ~63, (e.y1 + 63) & ~63 };
    if (r.x1 > w) r.x1 = w;
    if (r.y1 > h) r.y1 = h;
    return r;
}
__global__ __launch_bounds__(256) void yk_decall_render_blocks_batch_win_kernel(const DecBatch B, const DWinRect* __restrict__ wins, int w, int h, int latW, size_t planeSize,
                                                                                int tileW, int stride4) {
    const size_t f = blockIdx.y;
    yk_decall_render_blocks_body<true>(B.plans[f], w, h, latW, B.mapRGB + f * B.sMapRGB, B.planes + f * B.sPlanes, planeSize, tileW,
                                 reinterpret_cast<uint32_t*>(B.tile4 + f * B.sTile4), stride4, blockIdx.x, yk_bwin_rect64(wins[f], w, h));
}

// ---- partial planes: DecompressGradient4x4R / G / B / RG / GB / RB (decoder/YAIK_Gradient.cpp:1208-1226, :1420-2732) ------------
// `loaded` holds one bit per plane and lattice point (the three planes of mapRGBMask); the masks are split first (UpdateTileAndRGBMask).
__global__ void yk_dec_split_kernel(uint8_t* __restrict__ loaded, size_t lat, uint8_t* __restrict__ tile4, size_t tile4Size) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < lat) loaded[i] = (loaded[i] & 1) ? 7 : 0;                           // planes 1, 2 <- plane 0 (YAIK_API.cpp:536-537)
    if (i < tile4Size) { const uint8_t v = tile4[i]; tile4[tile4Size + i] = v; tile4[2 * tile4Size + i] = v; }     // :539-540
}
// 4x4 tiles: 32x32 swizzle blocks of 64 tiles, bit t -> tile (t % 8, t / 8)
__device__ __forceinline__ bool yk_d44_tile(const uint32_t* bitmap, size_t nBits, size_t pos, int w, int h, int& x, int& y) {
    if (pos >= nBits || !((bitmap[pos >> 5] >> (pos & 31)) & 1u)) return false;
    const int xBB = (w + 31) / 32;
    const uint32_t blk = (uint32_t)(pos >> 6), t = (uint32_t)(pos & 63);
    x = (int)(blk % xBB) * 32 + (int)(t & 7) * 4; y = (int)(blk / xBB) * 32 + (int)(t >> 3) * 4;
    return x < w && y < h;
}
__global__ __launch_bounds__(256) void yk_dec44p_owner_kernel(const uint32_t* __restrict__ bitmap, size_t nBits, int w, int h, int latW, int planeBit,
                                                              const uint8_t* __restrict__ loaded, uint32_t* __restrict__ owner) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int x, y;
    if (!yk_d44_tile(bitmap, nBits, pos, w, h, x, y)) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t li = (size_t)((y >> 2) + (k >> 1)) * latW + (x >> 2) + (k & 1);
        if ((~loaded[li]) & planeBit) atomicMin(&owner[li], ((uint32_t)pos << 2) | (uint32_t)k);      // some present plane still lacks this point
    }
}
// EMIT=false: bytes popped per workgroup of 1024 tile slots; EMIT=true: pop them (per corner TL,TR,BL,BR, per present plane in R,G,B
// order, only planes that lack the point, e.g. :1516-1580), then mark the point for the present planes
template <bool EMIT>
__global__ __launch_bounds__(1024) void yk_dec44p_corner_kernel(const uint32_t* __restrict__ bitmap, size_t nBits, int w, int h, int latW, int planeBit,
                                                                uint8_t* __restrict__ loaded, const uint32_t* __restrict__ owner, uint32_t* __restrict__ blockSums,
                                                                const uint8_t* __restrict__ rgb, size_t rgbBytes, uint8_t* __restrict__ mapRGB) {
    __shared__ uint32_t s_tmp[32];
    const size_t pos = (size_t)blockIdx.x * 1024 + threadIdx.x;
    int x = 0, y = 0;
    const bool set = yk_d44_tile(bitmap, nBits, pos, w, h, x, y);
    uint32_t need[4] = { 0, 0, 0, 0 }, bytes = 0;
    size_t li[4] = { 0, 0, 0, 0 };
    if (set) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            li[k] = (size_t)((y >> 2) + (k >> 1)) * latW + (x >> 2) + (k & 1);
            if (owner[li[k]] == (((uint32_t)pos << 2) | (uint32_t)k)) { need[k] = (uint32_t)((~loaded[li[k]]) & planeBit); bytes += (uint32_t)__popc(need[k]); }
        }
    }
    uint32_t tot;
    const uint32_t ex = yk_block_exscan(bytes, s_tmp, &tot);
    if (!EMIT) { if (threadIdx.x == 0) blockSums[blockIdx.x] = tot; return; }
    uint32_t off = blockSums[blockIdx.x] + ex;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!need[k]) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) if ((need[k] >> c) & 1u) { mapRGB[li[k] * 3 + c] = off < rgbBytes ? rgb[off] : 0; off++; }
    }
}
__global__ __launch_bounds__(256) void yk_dec44p_mark_kernel(const uint32_t* __restrict__ owner, size_t lat, int planeBit, uint8_t* __restrict__ loaded) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < lat && owner[i] != 0xFFFFFFFFu) loaded[i] |= (uint8_t)planeBit;    // every touched point now has the present planes
}
// fill (truncating integer bilinear, e.g. :1617-1640) + tile4x4Mask marking.  consistentMarks = 0 reproduces what the reference's loops
// do to the mask: R / G / B never mark, GB / RB put the B marks at tile4x4Mask + (tile4x4MaskSize >> 1) (:1678, :1924).
__global__ __launch_bounds__(256) void yk_dec44p_render_kernel(const uint32_t* __restrict__ bitmap, size_t nBits, int w, int h, int latW, int planeBit, int consistentMarks,
                                                               const uint8_t* __restrict__ mapRGB, uint8_t* __restrict__ planes, size_t planeSize, int tileW,
                                                               uint32_t* __restrict__ tile4, size_t tile4Size, int stride4) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int x, y;
    if (!yk_d44_tile(bitmap, nBits, pos, w, h, x, y)) return;
    const size_t l0 = (size_t)(y >> 2) * latW + (x >> 2);
    for (int c = 0; c < 3; c++) {
        if (!((planeBit >> c) & 1)) continue;
        const int TL = mapRGB[l0 * 3 + c], TR = mapRGB[(l0 + 1) * 3 + c], BL = mapRGB[(l0 + latW) * 3 + c], BR = mapRGB[(l0 + latW + 1) * 3 + c];
        uint8_t* o = planes + (size_t)c * planeSize + ((size_t)(y >> 3) * tileW + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7);
#pragma unroll
        for (int ty = 0; ty < 4; ty++) {
            const int L = TL * (4 - ty) + BL * ty, R = TR * (4 - ty) + BR * ty;
            uint32_t v4 = 0;
#pragma unroll
            for (int tx = 0; tx < 4; tx++) v4 |= (uint32_t)(((L * (4 - tx) + R * tx) >> 4) & 255) << (8 * tx);
            *reinterpret_cast<uint32_t*>(o + ty * 8) = v4;
        }
        size_t base;
        if (consistentMarks) base = tile4Size * c;
        else {
            if (planeBit == 1 || planeBit == 2 || planeBit == 4) continue;
            base = (c == 2) ? (tile4Size >> 1) : tile4Size * c;
        }
        const int cx = x >> 2, cy = y >> 2;
        const size_t byteIdx = base + (size_t)(cx >> 2) + (size_t)(cy >> 1) * stride4;
        const uint32_t bit = (uint32_t)((((cx >> 1) & 1) << 2) | ((cy & 1) << 1) | (cx & 1));
        atomicOr(&tile4[byteIdx >> 2], 1u << (bit + 8 * (byteIdx & 3)));
    }
}

// ---- 1-D range decode -------------------------------------------------------------------------------------------
// quadrant mask of tile i (bit set = quadrant already filled by a gradient tile, YAIK_3DTile.cpp:74-78); 0xF past the end
__device__ __forceinline__ int yk_d1_quads(const uint8_t* __restrict__ tile4, int stride4, int tilesW, size_t T8, size_t i) {
    if (i >= T8) return 0xF;
    const int tx = (int)(i % tilesW), ty = (int)(i / tilesW);
    const int q = tile4[(tx >> 1) + (size_t)ty * stride4];
    return (q >> ((tx & 1) ? 4 : 0)) & 0xF;
}
// coded tiles (low 11 bits) and pixel bytes (above) of a tile, packed so that one scan serves both: a block of 1024 tiles holds at
// most 1024 coded tiles and 65536 pixel bytes
__device__ __forceinline__ uint32_t yk_d1_packed_count(int q) { return (q != 0xF ? 1u : 0u) | ((16u * (4u - (uint32_t)__popc(q))) << 11); }

// per block of 1024 tiles: coded tiles and pixel bytes, from the mask alone
// (bodies as __device__ functions, shared with the batch kernels below: bx = blockIdx.x)
__device__ __forceinline__ void yk_dec1d_count_body(const uint8_t* __restrict__ tile4, int stride4, int tilesW, size_t T8,
                                                    uint32_t* __restrict__ blockTiles, uint32_t* __restrict__ blockPix, uint32_t* __restrict__ offInBlk, const uint32_t bx) {
    __shared__ uint32_t s_tmp[32];
    const size_t i = (size_t)bx * 1024 + threadIdx.x;
    uint32_t tot;
    const int q = yk_d1_quads(tile4, stride4, tilesW, T8, i);
    const uint32_t e = yk_block_exscan(yk_d1_packed_count(q), s_tmp, &tot);
    if (i < T8) offInBlk[i] = e | ((uint32_t)q << 28);                         // the tile's packed offsets inside its block (28 bits) + its quadrant mask
    if (threadIdx.x == 0) { blockTiles[bx] = tot & 2047u; blockPix[bx] = tot >> 11; }
}
__global__ __launch_bounds__(1024) void yk_dec1d_count_kernel(const uint8_t* __restrict__ tile4, int stride4, int tilesW, size_t T8,
                                                              uint32_t* __restrict__ blockTiles, uint32_t* __restrict__ blockPix, uint32_t* __restrict__ offInBlk) {
    yk_dec1d_count_body(tile4, stride4, tilesW, T8, blockTiles, blockPix, offInBlk, blockIdx.x);
}
// both block-sum arrays -> exclusive prefixes in place, totals[0] = coded tiles, totals[1] = pixel bytes (one launch)
__device__ __forceinline__ void yk_dec1d_scan_body(uint32_t* __restrict__ blockTiles, uint32_t* __restrict__ blockPix, int nBlocks, uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_tmp[32];
#pragma unroll 1
    for (int a = 0; a < 2; a++) {
        uint32_t* arr = a ? blockPix : blockTiles;
        uint32_t base = 0;
        // more than one trip needs more than 1024 scan blocks = 2^20 tiles, an image above 8192 x 8192: no test reaches the second trip
        for (int start = 0; start < nBlocks; start += 1024) {
            const int i = start + threadIdx.x;
            const uint32_t v = i < nBlocks ? arr[i] : 0u;
            uint32_t tot;
            const uint32_t e = yk_block_exscan(v, s_tmp, &tot);
            if (i < nBlocks) arr[i] = base + e;
            base += tot;
        }
        if (threadIdx.x == 0) totals[a] = base;
    }
}

__global__ __launch_bounds__(1024) void yk_dec1d_scan_kernel(uint32_t* __restrict__ blockTiles, uint32_t* __restrict__ blockPix, int nBlocks, uint32_t* __restrict__ totals) {
    yk_dec1d_scan_body(blockTiles, blockPix, nBlocks, totals);
}

// FOUR lanes per tile, one lane per pair of rows of one half of the tile; a tile's offsets in the type and pixel streams come from the count
// kernel's per-tile scan (offInBlk) + the scanned block sums, so the kernel is a plain stream: no workgroup scan, no barrier, every lane's loads
// independent of every other lane's (the first form scanned 1024 tiles per workgroup of 1024 threads and then walked them in four rounds: two
// resident workgroups per CU, each a chain of dependent round trips).  The stream holds a half's rows as [left quadrant 4 B][right quadrant
// 4 B] per row, absent quadrants left out (:95-124): with both quadrants present a row pair is 16 contiguous, 16-byte aligned stream bytes AND
// 16 contiguous bytes of the 8x8-tiled plane (one load, one store per lane, a wave moves 1 KB per instruction); with one quadrant it is an
// 8-byte load and two 4-byte stores.
#ifndef YK_D1_TPL
#define YK_D1_TPL 4
#endif
// WIN (a decode window, yk_decode_set_window): the lanes enumerate the window's tiles row-major, tile j of the window being tile
// (ty0 + j / wtW) * tilesW + tx0 + j % wtW of the image; T8 is then the window's tile count.  The 64 tiles of a round no longer lie in one scan
// block (a window row may end in one block and the next begin in another), so the two block bases are loaded per lane there.
struct D1Win { uint32_t tx0, ty0, wtW, tilesW; };
// LIST (a prepared image, yk_decode_render_windows_device): the lanes enumerate the 64 tiles of every 64x64 block of a list: tile j of the launch is
// tile (by * 8 + (j & 63) / 8, bx * 8 + (j & 7)) of block list[j >> 6] = (bx, by); T8 is then 64 x the list's length.  Tiles past the right or bottom
// edge of the image (a partial block) are inactive.  As under a window the two block bases are loaded per lane: on a 520-wide image one tile row of
// a block already straddles the boundary between two scan blocks.
struct D1List { const uint32_t* list; uint32_t xB64, tilesW, tilesH; };
enum { YK_D1_ALL = 0, YK_D1_WIN = 1, YK_D1_LIST = 2 };
template <int MODE>
__device__ __forceinline__ void yk_dec1d_body(const uint32_t* __restrict__ offInBlk, size_t T8,
                                              const uint32_t* __restrict__ baseTiles, const uint32_t* __restrict__ basePix,
                                              const uint32_t* __restrict__ totals /*[0]=tiles,[1]=pix*/, const uint8_t* __restrict__ type, size_t typeBytes,
                                              const uint8_t* __restrict__ pix, size_t pixBytes, int invRange,
                                              uint8_t* __restrict__ planes, size_t planeSize, int planeOverride, const uint32_t* __restrict__ runBase, const uint32_t bx,
                                              const D1Win wn = D1Win{ 0, 0, 1, 0 }, const D1List ls = D1List{ nullptr, 1, 0, 0 }) {
    constexpr bool WIN = MODE == YK_D1_WIN, LIST = MODE == YK_D1_LIST;
    // planeOverride < 0: the three planes share one mask (no partial-plane pass ran): plane = blockIdx.y, its streams start at
    // plane * totals.  Otherwise one plane per launch with its own mask, streams start at runBase (tiles, pixels of the planes before it).
    const int p = planeOverride < 0 ? (int)blockIdx.y : planeOverride;
    const size_t baseT = planeOverride < 0 ? (size_t)p * totals[0] : (size_t)runBase[0], baseP = planeOverride < 0 ? (size_t)p * totals[1] : (size_t)runBase[1];
    const int j = threadIdx.x & 3, half = j >> 1, rp = j & 1;
    uint8_t* const plane = planes + (size_t)p * planeSize;
    // YK_D1_TPL tiles per lane, 64 tiles apart (a wave's accesses stay contiguous), in three phases so that a lane's round trips overlap instead of
    // following each other: all offset words, then all parameter bytes and stream bytes, then the arithmetic and the stores.  (Tile after tile
    // a wave made eight dependent round trips; with eight waves per SIMD and 48 waves per SIMD to run, those chains were the launch's duration.)
    uint32_t ow[YK_D1_TPL];
    size_t ti[YK_D1_TPL];                                                       // WIN, LIST: the tile of the image that tile j of the launch is
    bool act[YK_D1_TPL];                                                        // LIST: ... and whether it lies inside the image
#pragma unroll
    for (int rep = 0; rep < YK_D1_TPL; rep++) {
        const size_t i = ((size_t)bx * YK_D1_TPL + rep) * 64 + (threadIdx.x >> 2);
        if (LIST) {
            const bool in = i < T8;
            const uint32_t b = in ? ls.list[i >> 6] : 0u, t = (uint32_t)i & 63u;
            const uint32_t by = b / ls.xB64, tx = (b - by * ls.xB64) * 8u + (t & 7u), ty = by * 8u + (t >> 3);
            act[rep] = in && tx < ls.tilesW && ty < ls.tilesH;
            ti[rep] = act[rep] ? (size_t)ty * ls.tilesW + tx : 0;
            ow[rep] = act[rep] ? offInBlk[ti[rep]] : 0xF0000000u;
        } else if (WIN) {
            const uint32_t jy = (uint32_t)i / wn.wtW, jx = (uint32_t)i - jy * wn.wtW;
            ti[rep] = i < T8 ? (size_t)(wn.ty0 + jy) * wn.tilesW + wn.tx0 + jx : 0;
            ow[rep] = i < T8 ? offInBlk[ti[rep]] : 0xF0000000u;
        } else
            ow[rep] = i < T8 ? offInBlk[i] : 0xF0000000u;                       // past the end: a tile with nothing to decode
    }
    int tb[YK_D1_TPL]; uint4 L[YK_D1_TPL]; bool coded[YK_D1_TPL], live[YK_D1_TPL];
#pragma unroll
    for (int rep = 0; rep < YK_D1_TPL; rep++) {
        const int q = (int)(ow[rep] >> 28);
        const int qh = (q >> (half * 2)) & 3;                                    // bit 0: left quadrant filled, bit 1: right
        // the 64 tiles of a workgroup's round lie in one scan block: its two bases are scalar loads
        const size_t blk = (WIN || LIST) ? ti[rep] >> 10 : (((size_t)bx * YK_D1_TPL + rep) * 64) >> 10;
        const bool inRange = LIST ? act[rep] : WIN ? ((size_t)bx * YK_D1_TPL + rep) * 64 + (threadIdx.x >> 2) < T8 : (((size_t)bx * YK_D1_TPL + rep) * 64) < T8;
        const uint32_t offT = (inRange ? baseTiles[blk] : 0u) + (ow[rep] & 2047u), offP = (inRange ? basePix[blk] : 0u) + ((ow[rep] >> 11) & 0x1FFFFu);
        const int nTop = 2 - (q & 1) - ((q >> 1) & 1);
        const size_t to = (baseT + offT) * 3;
        // the tile's three parameter bytes: one byte load per lane (lane j of the tile fetches byte min(j, 2)), handed round the quad by DPP below
        live[rep] = q != 0xF;                                                     // the tile has a quadrant nothing filled: it is written here, with zeros when its parameters are missing
        coded[rep] = live[rep] && to + 2 < typeBytes;
        tb[rep] = 0;
        if (coded[rep]) tb[rep] = type[to + (j < 2 ? j : 2)];
        L[rep] = make_uint4(0u, 0u, 0u, 0u);
        if (coded[rep] && qh == 0) {
            const size_t po = baseP + offP + (half ? 16 * nTop : 0) + (size_t)rp * 16;
            if (po + 16 <= pixBytes) L[rep] = *reinterpret_cast<const uint4*>(pix + po);
            else if (po < pixBytes) { uint32_t tmp[4] = { 0, 0, 0, 0 }; for (int k = 0; k < 4; k++) if (po + 4 * k + 3 < pixBytes) tmp[k] = *reinterpret_cast<const uint32_t*>(pix + po + 4 * k); L[rep] = make_uint4(tmp[0], tmp[1], tmp[2], tmp[3]); }
        } else if (coded[rep] && qh != 3) {
            const size_t po = baseP + offP + (half ? 16 * nTop : 0) + (size_t)rp * 8;
            if (po + 8 <= pixBytes) { const uint2 t2 = *reinterpret_cast<const uint2*>(pix + po); L[rep].x = t2.x; L[rep].y = t2.y; }
            else if (po + 3 < pixBytes) L[rep].x = *reinterpret_cast<const uint32_t*>(pix + po);
        }
    }
#pragma unroll
    for (int rep = 0; rep < YK_D1_TPL; rep++) {
        const size_t i = (WIN || LIST) ? ti[rep] : ((size_t)bx * YK_D1_TPL + rep) * 64 + (threadIdx.x >> 2);
        const int q = (int)(ow[rep] >> 28);
        const int qh = (q >> (half * 2)) & 3;
        const int color0 = __builtin_amdgcn_update_dpp(0, tb[rep], 0x00, 0xF, 0xF, true), base = __builtin_amdgcn_update_dpp(0, tb[rep], 0x55, 0xF, 0xF, true),
                  delta = __builtin_amdgcn_update_dpp(0, tb[rep], 0xAA, 0xF, 0xF, true);
        // a tile the stream does not reach decodes as color0 = 0 with every index 0: zeros.  (The planes are not cleared per frame any more: what no
        // gradient / LUT tile covered is written here, whatever the stream holds: yk_decode_begin.)
        if (qh == 3 || !live[rep]) continue;
        const int delta2 = ((delta * invRange) >> 8) + 1;                       // :66, :86
        // v = L ? base + (((L - 1) * delta2) >> 16) : color0 (:113-124), four pixels of a dword at a time: for L >= 1 the value is byte 2 of
        // K + L * delta2 with K = (base << 16) - delta2 (delta2 <= 255 * 65536 + 1 < 2^24 for every compressionRange 1..255 -- below 2^21 only
        // from range 8 up, 8355841 at range 2 -- and L a byte: a 24-bit multiply with the byte selected by the instruction, L * delta2 < 2^32;
        // the sum wraps at 32 bits, which byte 2 does not see: it is (base + (((L - 1) * delta2) >> 16)) & 255, the reference's store into a u8);
        // the bytes with L == 0 are found with the carry-free zero-byte mask and take color0.  4.5 operations per pixel instead of 8.
        // (Range 1 with delta >= 128 overflows delta * invRange here as in the reference: unspecified)
        const uint32_t Kc = ((uint32_t)base << 16) - (uint32_t)delta2, d2u = (uint32_t)delta2, c0x4 = (uint32_t)color0 * 0x01010101u;
        auto dec4 = [&](uint32_t L4) {
            uint32_t t0, t1, t2, t3;
            asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(t0) : "v"(L4), "v"(d2u));
            asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(t1) : "v"(L4), "v"(d2u));
            asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(t2) : "v"(L4), "v"(d2u));
            asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(t3) : "v"(L4), "v"(d2u));
            t0 += Kc; t1 += Kc; t2 += Kc; t3 += Kc;
            const uint32_t lo = __builtin_amdgcn_perm(t1, t0, 0x0C0C0602u), hi = __builtin_amdgcn_perm(t3, t2, 0x06020C0Cu);   // byte 2 of each
            const uint32_t dec = lo | hi;
            const uint32_t z = ~(((L4 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | L4 | 0x7F7F7F7Fu);                                       // 0x80 in every byte with L == 0
            const uint32_t m = (z >> 7) * 255u;
            return (dec & ~m) | (c0x4 & m);
        };
        uint8_t* const o = plane + i * 64 + (half * 4 + rp * 2) * 8;               // the lane's two rows: 16 contiguous bytes of the tile
        if (qh == 0) *reinterpret_cast<uint4*>(o) = make_uint4(dec4(L[rep].x), dec4(L[rep].y), dec4(L[rep].z), dec4(L[rep].w));
        else {
            const int side = qh & 1;                                             // left filled -> the present quadrant is the right one
            *reinterpret_cast<uint32_t*>(o + side * 4) = dec4(L[rep].x);
            *reinterpret_cast<uint32_t*>(o + 8 + side * 4) = dec4(L[rep].y);
        }
    }
}

__global__ __launch_bounds__(256) void yk_dec1d_kernel(const uint32_t* __restrict__ offInBlk, size_t T8,
                                                       const uint32_t* __restrict__ baseTiles, const uint32_t* __restrict__ basePix,
                                                       const uint32_t* __restrict__ totals /*[0]=tiles,[1]=pix*/, const uint8_t* __restrict__ type, size_t typeBytes,
                                                       const uint8_t* __restrict__ pix, size_t pixBytes, int invRange,
                                                       uint8_t* __restrict__ planes, size_t planeSize, int planeOverride, const uint32_t* __restrict__ runBase) {
    yk_dec1d_body<YK_D1_ALL>(offInBlk, T8, baseTiles, basePix, totals, type, typeBytes, pix, pixBytes, invRange, planes, planeSize, planeOverride, runBase, blockIdx.x);
}
// the shared-mask mode (plane = blockIdx.y) over the tiles of a decode window; nWin = its tile count
__global__ __launch_bounds__(256) void yk_dec1d_win_kernel(const uint32_t* __restrict__ offInBlk, size_t nWin, const D1Win wn,
                                                           const uint32_t* __restrict__ baseTiles, const uint32_t* __restrict__ basePix,
                                                           const uint32_t* __restrict__ totals, const uint8_t* __restrict__ type, size_t typeBytes,
                                                           const uint8_t* __restrict__ pix, size_t pixBytes, int invRange, uint8_t* __restrict__ planes, size_t planeSize) {
    yk_dec1d_body<YK_D1_WIN>(offInBlk, nWin, baseTiles, basePix, totals, type, typeBytes, pix, pixBytes, invRange, planes, planeSize, -1, (const uint32_t*)nullptr, blockIdx.x, wn);
}

// the shared-mask mode over the tiles of the blocks of a list (a prepared image); nTiles = 64 x the list's length
__global__ __launch_bounds__(256) void yk_dec1d_list_kernel(const uint32_t* __restrict__ offInBlk, size_t nTiles, const D1List ls,
                                                            const uint32_t* __restrict__ baseTiles, const uint32_t* __restrict__ basePix,
                                                            const uint32_t* __restrict__ totals, const uint8_t* __restrict__ type, size_t typeBytes,
                                                            const uint8_t* __restrict__ pix, size_t pixBytes, int invRange, uint8_t* __restrict__ planes, size_t planeSize) {
    yk_dec1d_body<YK_D1_LIST>(offInBlk, nTiles, baseTiles, basePix, totals, type, typeBytes, pix, pixBytes, invRange, planes, planeSize, -1, (const uint32_t*)nullptr, blockIdx.x,
                              D1Win{ 0, 0, 1, 0 }, ls);
}

// ---- the 1-D chunk over a batch: the same three launches, frame = blockIdx.y (count), blockIdx.x (scan: one workgroup per frame), blockIdx.z
// (decode: blockIdx.y stays the plane).  A frame's streams (pointers and lengths) come from a table in HBM; its mask, planes and scratch arrays
// lie at base + f * stride.  The masks of a batch are never split (plane-subset chunks are refused), so the three planes share one count and scan.
struct D1Frame { const uint8_t* type; const uint8_t* pix; unsigned long long typeBytes, pixBytes; };
struct D1Batch {
    const D1Frame* frames;
    const uint8_t* tile4; uint8_t* planes; uint8_t* scratch;
    size_t sTile4, sPlanes, sScratch;
    size_t oBT, oBP, oTot, oOff;
};
__device__ __forceinline__ uint32_t* yk_d1batch_u32(const D1Batch& B, size_t f, size_t off) { return reinterpret_cast<uint32_t*>(B.scratch + f * B.sScratch + off); }

__global__ __launch_bounds__(1024) void yk_dec1d_count_batch_kernel(const D1Batch B, int stride4, int tilesW, size_t T8) {
    const size_t f = blockIdx.y;
    yk_dec1d_count_body(B.tile4 + f * B.sTile4, stride4, tilesW, T8, yk_d1batch_u32(B, f, B.oBT), yk_d1batch_u32(B, f, B.oBP), yk_d1batch_u32(B, f, B.oOff), blockIdx.x);
}
__global__ __launch_bounds__(1024) void yk_dec1d_scan_batch_kernel(const D1Batch B, int nBlocks) {
    const size_t f = blockIdx.x;
    yk_dec1d_scan_body(yk_d1batch_u32(B, f, B.oBT), yk_d1batch_u32(B, f, B.oBP), nBlocks, yk_d1batch_u32(B, f, B.oTot));
}
__global__ __launch_bounds__(256) void yk_dec1d_batch_kernel(const D1Batch B, size_t T8, int invRange, size_t planeSize) {
    const size_t f = blockIdx.z;
    const D1Frame& fr = B.frames[f];
    yk_dec1d_body<YK_D1_ALL>(yk_d1batch_u32(B, f, B.oOff), T8, yk_d1batch_u32(B, f, B.oBT), yk_d1batch_u32(B, f, B.oBP), yk_d1batch_u32(B, f, B.oTot), fr.type, (size_t)fr.typeBytes,
                  fr.pix, (size_t)fr.pixBytes, invRange, B.planes + f * B.sPlanes, planeSize, -1, (const uint32_t*)nullptr, blockIdx.x);
}
// ... with a window per frame (yk_decode_set_batch_windows): the tiles of frame f's window, its origin from the table; the windows of a batch have
// one size, so nWin, wtW and the grid are every frame's
__global__ __launch_bounds__(256) void yk_dec1d_batch_win_kernel(const D1Batch B, const DWinRect* __restrict__ wins, size_t nWin, uint32_t wtW, uint32_t tilesW, int invRange,
                                                                 size_t planeSize) {
    const size_t f = blockIdx.z;
    const D1Frame& fr = B.frames[f];
    const D1Win wn = { (uint32_t)wins[f].x0 >> 3, (uint32_t)wins[f].y0 >> 3, wtW, tilesW };
    yk_dec1d_body<YK_D1_WIN>(yk_d1batch_u32(B, f, B.oOff), nWin, yk_d1batch_u32(B, f, B.oBT), yk_d1batch_u32(B, f, B.oBP), yk_d1batch_u32(B, f, B.oTot), fr.type, (size_t)fr.typeBytes,
                  fr.pix, (size_t)fr.pixBytes, invRange, B.planes + f * B.sPlanes, planeSize, -1, (const uint32_t*)nullptr, blockIdx.x, wn);
}
// ... with a rectangle per frame (yk_decode_set_batch_rects): wins[f] is the rectangle's own 8-aligned cover, so the tile counts differ
// from frame to frame.  The grid is the largest cover's; a workgroup past its frame's count leaves before it loads anything (the body has no barrier).
__global__ __launch_bounds__(256) void yk_dec1d_batch_rects_kernel(const D1Batch B, const DWinRect* __restrict__ wins, uint32_t tilesW, int invRange, size_t planeSize) {
    const size_t f = blockIdx.z;
    const DWinRect wr = wins[f];
    const uint32_t wtW = (uint32_t)(wr.x1 - wr.x0) >> 3, nWin = wtW * ((uint32_t)(wr.y1 - wr.y0) >> 3);
    if (blockIdx.x * (uint32_t)(64 * YK_D1_TPL) >= nWin) return;
    const D1Frame& fr = B.frames[f];
    const D1Win wn = { (uint32_t)wr.x0 >> 3, (uint32_t)wr.y0 >> 3, wtW, tilesW };
    yk_dec1d_body<YK_D1_WIN>(yk_d1batch_u32(B, f, B.oOff), (size_t)nWin, yk_d1batch_u32(B, f, B.oBT), yk_d1batch_u32(B, f, B.oBP), yk_d1batch_u32(B, f, B.oTot), fr.type,
                  (size_t)fr.typeBytes, fr.pix, (size_t)fr.pixBytes, invRange, B.planes + f * B.sPlanes, planeSize, -1, (const uint32_t*)nullptr, blockIdx.x, wn);
}

__global__ void yk_dec_mask_kernel(const uint8_t* __restrict__ bits, int bw, int bh, unsigned long long* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bw * bh) return;
    const int x = i % bw, y = i / bw;
    const unsigned long long v = (bits[i >> 3] & (1 << (i & 7))) ? ~0ULL : 0ULL;     // YAIK_Mipmap.cpp:119-136
    unsigned long long* A = out + (size_t)y * 4 * bw + 2 * x;
    A[0] = v; A[1] = v; A[2 * bw] = v; A[2 * bw + 1] = v;
}

// a20: the default image builder (decoder/YAIK_DefaultCallback.cpp:24-191) and its device form: the 8x8-tiled planes -> 8-bit pixels at any
// address and pitch.  Pixel (x, y) channel k lands at out[y * rowBytes + x * C + k] (HWC: the builder's RGB888 / RGBA8888 rows) or at
// out[k * planeBytes + y * rowBytes + x] (CHW), C = 3 or 4.  The 4th channel is the alpha plane (stride strideA) or a constant.  With an alpha
// plane the reference never advances past the alpha byte (:53-60) and produces 3-byte-strided garbage; this kernel writes proper RGBA
// (4 B/pixel) instead, which is what YAIK.h documents.  Only pixel bytes are written: row padding and the bytes between planes are not touched.
// The planes are one linear array of tiles (64 B each, tile t = (tx, ty) at t = ty * tileW + tx).  A work unit is 16 consecutive tiles,
// 1 KB per plane: lane l loads bytes 16l..16l+15 of each plane (rows 2(l&3), 2(l&3)+1 of tile 16u + (l>>2)), so every load instruction is
// one dense 1 KB access, and writes its two 8-pixel row segments.  For a fixed l&3 the 16 lanes hold 16 consecutive tiles, so the stores of
// a row pair fill four runs of 16 * 8 * C bytes (HWC).  A lane derives its own (tx, ty), so a run may wrap into the next row of tiles.
// No LDS, no shuffles; w and h are multiples of 8, so only the last unit is partial.  A lane issues the loads of K units before its first store.
// Stores and alpha loads go through byte pointers (__builtin_memcpy): gfx950 runs with unaligned global access enabled and hipcc emits
// global_store_dwordx4 + dwordx2 per RGB segment, 2 x dwordx4 per RGBA segment, dwordx2 per CHW row and global_load_dwordx2 per alpha row for
// them (checked in the ISA), the fewest instructions those bytes allow; so one path serves every base and pitch.
#define YK_DT_THREADS 256
#define YK_DT_K 4                                   // units per lane in flight
#define YK_DT_TILES (YK_DT_THREADS / 4 * YK_DT_K)   // tiles per workgroup

enum { YK_DT_ALPHA_NONE = 0, YK_DT_ALPHA_PLANE = 1, YK_DT_ALPHA_CONST = 2 };

struct YkDetileArgs {
    const uint8_t* planes; size_t planeSize;         // R, G, B at planes + p * planeSize
    const uint8_t* alpha; size_t strideA;            // YK_DT_ALPHA_PLANE: row y at alpha + y * strideA
    uint32_t alphaConst;                             // YK_DT_ALPHA_CONST: the byte in all four lanes of a dword
    uint8_t* out; size_t rowBytes, planeBytes;
    uint32_t tileW, nTiles;
};

typedef uint32_t yk_dt4 __attribute__((ext_vector_type(4)));

// row segment of 8 pixels (dwords lo, hi of each plane) -> its bytes at o (HWC) or o + k * planeBytes (CHW)
template <int C, bool PLANAR>
__device__ __forceinline__ void yk_dt_emit(uint8_t* o, size_t planeBytes, uint32_t r0, uint32_t r1, uint32_t g0, uint32_t g1, uint32_t b0, uint32_t b1,
                                           uint32_t a0, uint32_t a1) {
    if constexpr (PLANAR) {
        const uint32_t v[4][2] = { { r0, r1 }, { g0, g1 }, { b0, b1 }, { a0, a1 } };
#pragma unroll
        for (int k = 0; k < C; k++) __builtin_memcpy(o + (size_t)k * planeBytes, v[k], 8);
    } else if constexpr (C == 3) {
        // 4 pixels of R, G, B dwords -> 12 bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        uint32_t wd[6];
        const uint32_t rg[2][2] = { { __builtin_amdgcn_perm(g0, r0, 0x05010400u), __builtin_amdgcn_perm(g0, r0, 0x07030602u) },
                                    { __builtin_amdgcn_perm(g1, r1, 0x05010400u), __builtin_amdgcn_perm(g1, r1, 0x07030602u) } };
        const uint32_t bb[2] = { b0, b1 }, gg[2] = { g0, g1 };
#pragma unroll
        for (int h = 0; h < 2; h++) {
            wd[3 * h + 0] = __builtin_amdgcn_perm(bb[h], rg[h][0], 0x02040100u);
            wd[3 * h + 1] = __builtin_amdgcn_perm(rg[h][1], __builtin_amdgcn_perm(bb[h], gg[h], 0x05010400u), 0x05040302u);
            wd[3 * h + 2] = __builtin_amdgcn_perm(bb[h], rg[h][1], 0x07030206u);
        }
        __builtin_memcpy(o, wd, 24);
    } else {
        // 4 pixels of R, G, B, A dwords -> 16 bytes r g b a x 4
        yk_dt4 px[2];
        const uint32_t rr[2] = { r0, r1 }, gg[2] = { g0, g1 }, bb[2] = { b0, b1 }, aa[2] = { a0, a1 };
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t rgL = __builtin_amdgcn_perm(gg[h], rr[h], 0x05010400u), rgH = __builtin_amdgcn_perm(gg[h], rr[h], 0x07030602u);
            const uint32_t baL = __builtin_amdgcn_perm(aa[h], bb[h], 0x05010400u), baH = __builtin_amdgcn_perm(aa[h], bb[h], 0x07030602u);
            px[h] = yk_dt4{ __builtin_amdgcn_perm(baL, rgL, 0x05040100u), __builtin_amdgcn_perm(baL, rgL, 0x07060302u),
                            __builtin_amdgcn_perm(baH, rgH, 0x05040100u), __builtin_amdgcn_perm(baH, rgH, 0x07060302u) };
        }
        __builtin_memcpy(o, px, 32);
    }
}

struct YkDtUnit { yk_dt4 r, g, b; uint32_t a[4]; size_t o; };

// A decode window (yk_decode_set_window) in tiles: tile (tx0 + jx, ty0 + jy) of the planes goes to pixel (8 jx, 8 jy) of the destination.  The
// window forms walk the window's wtW x wtH tiles row-major (a.nTiles = their count; a.alpha points at the window's first alpha byte).
struct YkDetileWin { uint32_t tx0, ty0, wtW; };

template <int C, bool PLANAR, int ASRC>
__device__ __forceinline__ void yk_dt_load(const YkDetileArgs& a, uint32_t t, uint32_t rp, YkDtUnit& u) {
    const size_t ti = (size_t)t * 64 + rp * 16;
    u.r = *reinterpret_cast<const yk_dt4*>(a.planes + ti);
    u.g = *reinterpret_cast<const yk_dt4*>(a.planes + a.planeSize + ti);
    u.b = *reinterpret_cast<const yk_dt4*>(a.planes + 2 * a.planeSize + ti);
    const uint32_t ty = t / a.tileW, tx = t - ty * a.tileW;
    const size_t y = (size_t)ty * 8 + rp * 2, x = (size_t)tx * 8;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) {
        __builtin_memcpy(&u.a[0], a.alpha + y * a.strideA + x, 8);
        __builtin_memcpy(&u.a[2], a.alpha + (y + 1) * a.strideA + x, 8);
    }
    u.o = y * a.rowBytes + x * (PLANAR ? 1 : C);
}
// window tile j = (jx, jy): the planes are read at tile (tx0 + jx, ty0 + jy), alpha and destination are addressed by (jx, jy)
template <int C, bool PLANAR, int ASRC>
__device__ __forceinline__ void yk_dt_load_win(const YkDetileArgs& a, const YkDetileWin& wn, uint32_t j, uint32_t rp, YkDtUnit& u) {
    const uint32_t jy = j / wn.wtW, jx = j - jy * wn.wtW;
    const size_t ti = ((size_t)(wn.ty0 + jy) * a.tileW + wn.tx0 + jx) * 64 + rp * 16;
    u.r = *reinterpret_cast<const yk_dt4*>(a.planes + ti);
    u.g = *reinterpret_cast<const yk_dt4*>(a.planes + a.planeSize + ti);
    u.b = *reinterpret_cast<const yk_dt4*>(a.planes + 2 * a.planeSize + ti);
    const size_t y = (size_t)jy * 8 + rp * 2, x = (size_t)jx * 8;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) {
        __builtin_memcpy(&u.a[0], a.alpha + y * a.strideA + x, 8);
        __builtin_memcpy(&u.a[2], a.alpha + (y + 1) * a.strideA + x, 8);
    }
    u.o = y * a.rowBytes + x * (PLANAR ? 1 : C);
}

template <int C, bool PLANAR, int ASRC>
__device__ __forceinline__ void yk_dt_store(const YkDetileArgs& a, const YkDtUnit& u) {
    uint32_t al[4];
#pragma unroll
    for (int i = 0; i < 4; i++) al[i] = ASRC == YK_DT_ALPHA_PLANE ? u.a[i] : a.alphaConst;
    uint8_t* o = a.out + u.o;
    yk_dt_emit<C, PLANAR>(o, a.planeBytes, u.r.x, u.r.y, u.g.x, u.g.y, u.b.x, u.b.y, al[0], al[1]);
    yk_dt_emit<C, PLANAR>(o + a.rowBytes, a.planeBytes, u.r.z, u.r.w, u.g.z, u.g.w, u.b.z, u.b.w, al[2], al[3]);
}

template <int C, bool PLANAR, int ASRC>
__device__ __forceinline__ void yk_dec_detile_body(const YkDetileArgs& a, const uint32_t bx) {
    const uint32_t lane = threadIdx.x & 63, rp = lane & 3;
    // unit of step k: blockIdx.x * K * 4 + k * 4 + wave, so the four waves of a workgroup stream 4 KB of every plane per step
    const uint32_t t0 = (bx * (YK_DT_K * 4) + (threadIdx.x >> 6)) * 16 + (lane >> 2);
    if ((bx + 1) * (uint32_t)YK_DT_TILES <= a.nTiles) {
        YkDtUnit u[YK_DT_K];                                                  // every unit of the workgroup exists: all loads first
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) yk_dt_load<C, PLANAR, ASRC>(a, t0 + k * 64, rp, u[k]);
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) yk_dt_store<C, PLANAR, ASRC>(a, u[k]);
        return;
    }
    for (int k = 0; k < YK_DT_K; k++) {                                       // the last workgroup: tiles up to nTiles
        const uint32_t t = t0 + k * 64;
        if (t >= a.nTiles) continue;
        YkDtUnit u;
        yk_dt_load<C, PLANAR, ASRC>(a, t, rp, u);
        yk_dt_store<C, PLANAR, ASRC>(a, u);
    }
}

template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_kernel(YkDetileArgs a) {
    yk_dec_detile_body<C, PLANAR, ASRC>(a, blockIdx.x);
}
// the window form: the same lanes and steps over the window's tiles (a row of the window is contiguous in the planes, rows are tileW tiles apart)
template <int C, bool PLANAR, int ASRC>
__device__ __forceinline__ void yk_dec_detile_win_body(const YkDetileArgs a, const YkDetileWin wn, const uint32_t bx) {
    const uint32_t lane = threadIdx.x & 63, rp = lane & 3;
    const uint32_t j0 = (bx * (YK_DT_K * 4) + (threadIdx.x >> 6)) * 16 + (lane >> 2);
    if ((bx + 1) * (uint32_t)YK_DT_TILES <= a.nTiles) {
        YkDtUnit u[YK_DT_K];
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) yk_dt_load_win<C, PLANAR, ASRC>(a, wn, j0 + k * 64, rp, u[k]);
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) yk_dt_store<C, PLANAR, ASRC>(a, u[k]);
        return;
    }
    for (int k = 0; k < YK_DT_K; k++) {
        const uint32_t j = j0 + k * 64;
        if (j >= a.nTiles) continue;
        YkDtUnit u;
        yk_dt_load_win<C, PLANAR, ASRC>(a, wn, j, rp, u);
        yk_dt_store<C, PLANAR, ASRC>(a, u);
    }
}
template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_win_kernel(YkDetileArgs a, const YkDetileWin wn) {
    yk_dec_detile_win_body<C, PLANAR, ASRC>(a, wn, blockIdx.x);
}
// K windows of one size of a prepared image (yk_decode_render_windows_device): window blockIdx.y, its origin (pixels) from a table in HBM, goes to
// a.out + k * windowBytes; a.alpha (YK_DT_ALPHA_PLANE) is the whole plane and is read at the window's own offset
template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_wins_kernel(YkDetileArgs a, const int* __restrict__ xy, uint32_t wtW, size_t windowBytes) {
    const uint32_t k = blockIdx.y;
    const uint32_t x0 = (uint32_t)xy[2 * k], y0 = (uint32_t)xy[2 * k + 1];
    a.out += (size_t)k * windowBytes;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) a.alpha += (size_t)y0 * a.strideA + x0;
    const YkDetileWin wn = { x0 >> 3, y0 >> 3, wtW };
    yk_dec_detile_win_body<C, PLANAR, ASRC>(a, wn, blockIdx.x);
}
template <int C, bool PLANAR, int ASRC>
static void yk_dt_launch_wins(const YkDetileArgs& a, hipStream_t s, int nWindows, const int* devXY, uint32_t wtW, size_t windowBytes) {
    const unsigned gx = (a.nTiles + YK_DT_TILES - 1) / YK_DT_TILES;
    hipLaunchKernelGGL((yk_dec_detile_wins_kernel<C, PLANAR, ASRC>), dim3(gx, (unsigned)nWindows), dim3(YK_DT_THREADS), 0, s, a, devXY, wtW, windowBytes);
}
// a batch: frame blockIdx.y's planes at a.planes + f * planesFrame, its pixels at a.out + f * outFrame
// (YK_DT_ALPHA_PLANE: its alpha plane at a.alpha + f * alphaFrame, the planes of yk_decode_alpha_batch_device)
template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_batch_kernel(YkDetileArgs a, size_t planesFrame, size_t outFrame, size_t alphaFrame) {
    a.planes += (size_t)blockIdx.y * planesFrame; a.out += (size_t)blockIdx.y * outFrame;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) a.alpha += (size_t)blockIdx.y * alphaFrame;
    yk_dec_detile_body<C, PLANAR, ASRC>(a, blockIdx.x);
}
// a batch with a window per frame (yk_decode_set_batch_windows): frame blockIdx.y's window, its origin from the table in HBM, goes to
// a.out + f * outFrame as a.nTiles = wtW x wtH tiles; YK_DT_ALPHA_PLANE reads frame f's whole alpha plane at the window's own offset
template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_batch_win_kernel(YkDetileArgs a, const DWinRect* __restrict__ wins, uint32_t wtW, size_t planesFrame,
                                                                                size_t outFrame, size_t alphaFrame) {
    const uint32_t f = blockIdx.y;
    const uint32_t x0 = (uint32_t)wins[f].x0, y0 = (uint32_t)wins[f].y0;
    a.planes += (size_t)f * planesFrame; a.out += (size_t)f * outFrame;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) a.alpha += (size_t)f * alphaFrame + (size_t)y0 * a.strideA + x0;
    const YkDetileWin wn = { x0 >> 3, y0 >> 3, wtW };
    yk_dec_detile_win_body<C, PLANAR, ASRC>(a, wn, blockIdx.x);
}
template <int C, bool PLANAR, int ASRC>
static void yk_dt_launch_batch_win(const YkDetileArgs& a, hipStream_t s, int nFrames, const DWinRect* wins, uint32_t wtW, size_t planesFrame, size_t outFrame, size_t alphaFrame) {
    const unsigned gx = (a.nTiles + YK_DT_TILES - 1) / YK_DT_TILES;
    hipLaunchKernelGGL((yk_dec_detile_batch_win_kernel<C, PLANAR, ASRC>), dim3(gx, (unsigned)nFrames), dim3(YK_DT_THREADS), 0, s, a, wins, wtW, planesFrame, outFrame, alphaFrame);
}

// ---- the clipping forms: windows at any pixel offset and size (yk_decode_set_window_px and its kin, yk_window_px.h) -----------------
// The window forms above over the tiles of the window's 8-aligned COVER: the same lanes, units, steps and loads (dense 16-byte loads per lane,
// all loads of a workgroup before its first store; the cover lies inside the image, so the 8-byte alpha loads of a cover tile stay inside the
// plane).  Only the store differs.  Pixel (X, Y) of the cover is pixel (X - dx, Y - dy) of the ww x wh destination: a row outside [0, wh) is
// skipped, a segment wholly inside [0, ww) goes through yk_dt_emit at its shifted address (unaligned, which that path serves), a segment the
// left or right edge cuts -- the first and last tile column of a cover, and the columns before dx of a shared cover -- is written pixel by
// pixel.  Rows and columns are clipped by the one function the CPU tool checks exhaustively (yk_wpx_clip), so no byte outside the pixels is written.
struct YkDetileClip { int dx, dy, ww, wh; };

// columns src0 .. src0 + n - 1 (n < 8) of a row segment -> their bytes from o on.  CHW: the kept bytes of a plane are one run, written as at most
// a dword, a word and a byte; HWC: a predicated store per pixel (a dword, or a word and a byte), the pixel's bytes picked by constant shifts
template <int C, bool PLANAR>
__device__ __forceinline__ void yk_dt_emit_px(uint8_t* o, size_t planeBytes, int src0, int n, uint32_t r0, uint32_t r1, uint32_t g0, uint32_t g1, uint32_t b0, uint32_t b1,
                                              uint32_t a0, uint32_t a1) {
    if constexpr (PLANAR) {
        const uint64_t v[4] = { r0 | (uint64_t)r1 << 32, g0 | (uint64_t)g1 << 32, b0 | (uint64_t)b1 << 32, a0 | (uint64_t)a1 << 32 };
#pragma unroll
        for (int k = 0; k < C; k++) {
            uint64_t t = v[k] >> (8 * src0);
            uint8_t* p = o + (size_t)k * planeBytes;
            if (n & 4) { const uint32_t d = (uint32_t)t; __builtin_memcpy(p, &d, 4); t >>= 32; p += 4; }
            if (n & 2) { const uint16_t d = (uint16_t)t; __builtin_memcpy(p, &d, 2); t >>= 16; p += 2; }
            if (n & 1) *p = (uint8_t)t;
        }
    } else {
        const uint32_t rr[2] = { r0, r1 }, gg[2] = { g0, g1 }, bb[2] = { b0, b1 }, aa[2] = { a0, a1 };
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (i < src0 || i >= src0 + n) continue;
            const int sh = 8 * (i & 3);
            const uint32_t r = (rr[i >> 2] >> sh) & 255u, g = (gg[i >> 2] >> sh) & 255u, b = (bb[i >> 2] >> sh) & 255u;
            uint8_t* p = o + (i - src0) * C;
            if constexpr (C == 4) {
                const uint32_t d = r | g << 8 | b << 16 | ((aa[i >> 2] >> sh) & 255u) << 24;
                __builtin_memcpy(p, &d, 4);
            } else {
                const uint16_t d = (uint16_t)(r | g << 8);
                __builtin_memcpy(p, &d, 2);
                p[2] = (uint8_t)b;
            }
        }
    }
}
// the two rows of cover tile (jx, jy) this lane holds, clipped against the window
template <int C, bool PLANAR, int ASRC>
__device__ __forceinline__ void yk_dt_store_px(const YkDetileArgs& a, const YkDetileClip& cl, const YkDtUnit& u, uint32_t jx, uint32_t jy, uint32_t rp) {
    const YkPxClip kx = yk_wpx_clip((int)jx, cl.dx, cl.ww), ky = yk_wpx_clip((int)jy, cl.dy, cl.wh);
    if (kx.n == 0 || ky.n == 0) return;
    uint32_t al[4];
#pragma unroll
    for (int i = 0; i < 4; i++) al[i] = ASRC == YK_DT_ALPHA_PLANE ? u.a[i] : a.alphaConst;
    const uint32_t rr[4] = { u.r.x, u.r.y, u.r.z, u.r.w }, gg[4] = { u.g.x, u.g.y, u.g.z, u.g.w }, bb[4] = { u.b.x, u.b.y, u.b.z, u.b.w };
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int row = (int)rp * 2 + i;                                      // of the tile
        if (row < ky.src0 || row >= ky.src0 + ky.n) continue;
        uint8_t* o = a.out + (size_t)(ky.dst + row - ky.src0) * a.rowBytes + (size_t)kx.dst * (PLANAR ? 1 : C);
        if (kx.n == 8) yk_dt_emit<C, PLANAR>(o, a.planeBytes, rr[2 * i], rr[2 * i + 1], gg[2 * i], gg[2 * i + 1], bb[2 * i], bb[2 * i + 1], al[2 * i], al[2 * i + 1]);
        else yk_dt_emit_px<C, PLANAR>(o, a.planeBytes, kx.src0, kx.n, rr[2 * i], rr[2 * i + 1], gg[2 * i], gg[2 * i + 1], bb[2 * i], bb[2 * i + 1], al[2 * i], al[2 * i + 1]);
    }
}
// wn: the cover in tiles; a.nTiles its tile count; a.alpha (YK_DT_ALPHA_PLANE) points at the cover's first alpha byte
template <int C, bool PLANAR, int ASRC>
__device__ __forceinline__ void yk_dec_detile_win_px_body(const YkDetileArgs a, const YkDetileWin wn, const YkDetileClip cl, const uint32_t bx) {
    const uint32_t lane = threadIdx.x & 63, rp = lane & 3;
    const uint32_t j0 = (bx * (YK_DT_K * 4) + (threadIdx.x >> 6)) * 16 + (lane >> 2);
    if ((bx + 1) * (uint32_t)YK_DT_TILES <= a.nTiles) {
        YkDtUnit u[YK_DT_K];
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) yk_dt_load_win<C, PLANAR, ASRC>(a, wn, j0 + k * 64, rp, u[k]);
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) {
            const uint32_t j = j0 + k * 64, jy = j / wn.wtW;
            yk_dt_store_px<C, PLANAR, ASRC>(a, cl, u[k], j - jy * wn.wtW, jy, rp);
        }
        return;
    }
    for (int k = 0; k < YK_DT_K; k++) {
        const uint32_t j = j0 + k * 64, jy = j / wn.wtW;
        if (j >= a.nTiles) continue;
        YkDtUnit u;
        yk_dt_load_win<C, PLANAR, ASRC>(a, wn, j, rp, u);
        yk_dt_store_px<C, PLANAR, ASRC>(a, cl, u, j - jy * wn.wtW, jy, rp);
    }
}
// one pixel window of the image begun (yk_decode_set_window_px)
template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_win_px_kernel(YkDetileArgs a, const YkDetileWin wn, const YkDetileClip cl) {
    yk_dec_detile_win_px_body<C, PLANAR, ASRC>(a, wn, cl, blockIdx.x);
}
// K pixel windows of ww x wh of a prepared image of w x h (yk_decode_render_windows_px_device): window blockIdx.y's pixel origin from the table in
// HBM, its shared cover (one size for every origin, a.nTiles tiles) worked out here by the functions that sized the launch
template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_wins_px_kernel(YkDetileArgs a, const int* __restrict__ xy, int ww, int wh, int w, int h, size_t windowBytes) {
    const uint32_t k = blockIdx.y;
    const int x0 = xy[2 * k], y0 = xy[2 * k + 1];
    const YkPxCover cx = yk_wpx_shared_cover(x0, ww, w), cy = yk_wpx_shared_cover(y0, wh, h);
    a.out += (size_t)k * windowBytes;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) a.alpha += (size_t)cy.c0 * a.strideA + (size_t)cx.c0;
    const YkDetileWin wn = { (uint32_t)cx.c0 >> 3, (uint32_t)cy.c0 >> 3, (uint32_t)cx.cw >> 3 };
    yk_dec_detile_win_px_body<C, PLANAR, ASRC>(a, wn, YkDetileClip{ x0 - cx.c0, y0 - cy.c0, ww, wh }, blockIdx.x);
}
// a batch with a pixel window per frame (yk_decode_set_batch_windows_px): wins[f] is frame f's cover (what the upstream kernels decoded), off[2f],
// off[2f + 1] the window's offset inside it
template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_batch_win_px_kernel(YkDetileArgs a, const DWinRect* __restrict__ wins, const int* __restrict__ off, uint32_t wtW,
                                                                                   int ww, int wh, size_t planesFrame, size_t outFrame, size_t alphaFrame) {
    const uint32_t f = blockIdx.y;
    const uint32_t x0 = (uint32_t)wins[f].x0, y0 = (uint32_t)wins[f].y0;
    a.planes += (size_t)f * planesFrame; a.out += (size_t)f * outFrame;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) a.alpha += (size_t)f * alphaFrame + (size_t)y0 * a.strideA + x0;
    const YkDetileWin wn = { x0 >> 3, y0 >> 3, wtW };
    yk_dec_detile_win_px_body<C, PLANAR, ASRC>(a, wn, YkDetileClip{ off[2 * f], off[2 * f + 1], ww, wh }, blockIdx.x);
}
// the template space of the de-tile kernels, for the launches of the clipping forms: f(tag) with tag.c, tag.planar, tag.asrc
template <int C, bool PLANAR, int ASRC> struct YkDtTag { static constexpr int c = C; static constexpr bool planar = PLANAR; static constexpr int asrc = ASRC; };
template <typename F>
static void yk_dt_each(int channels, bool planar, bool fromPlane, F f) {
    if (channels == 3) { if (planar) f(YkDtTag<3, true, YK_DT_ALPHA_NONE>{}); else f(YkDtTag<3, false, YK_DT_ALPHA_NONE>{}); }
    else if (fromPlane) { if (planar) f(YkDtTag<4, true, YK_DT_ALPHA_PLANE>{}); else f(YkDtTag<4, false, YK_DT_ALPHA_PLANE>{}); }
    else { if (planar) f(YkDtTag<4, true, YK_DT_ALPHA_CONST>{}); else f(YkDtTag<4, false, YK_DT_ALPHA_CONST>{}); }
}

// ---- the normalising form: fp16 / bf16 / fp32 elements, per-frame mirror (yk_decode_output_norm_device and its kin) ------------------
// The clipping forms above with another store: the same lanes, units, steps and loads, the alpha plane read at the cover's offset.  One kernel form
// serves every call: the per-frame cover and clip of yk_dec_detile_batch_win_px_kernel, where a whole frame is a cover at (0, 0) with ww x wh = w x h,
// an aligned window a cover with offset (0, 0) and a single image a batch of one; the cover, the offset and the mirror flag come from tables in HBM
// where the call has them and from the arguments where it has not.  Every decoded byte v of channel k becomes
//     f = fp32_add_rn(fp32_mul_rn((float)v, scale[k]), bias[k])          two roundings: contraction is off in yk_dn_value
// stored as fp32, or rounded to nearest even to fp16 / bf16 (the casts below; gfx950 has v_cvt_pk_bf16_f32).  A mirrored row segment is reversed in
// registers (column c -> 7 - c: the two dwords of a plane swapped and byte-reversed) and stored at the mirrored address yk_wpx_clip_mirror gives, so
// everything after the reversal is the unmirrored path.  A whole segment is one run of 8 C elements (HWC) or 8 elements per plane (CHW), stored
// through byte pointers like yk_dt_emit: 16-byte stores wherever the count allows (fp16 CHW row: one dwordx4; fp32 HWC4: eight).  A cut segment
// is stored pixel by pixel.  Pitches are in bytes and multiples of the element size.
struct YkDetileNorm {
    float scale[4], bias[4];
    uint32_t cx0, cy0;                                // the cover's origin in the planes (pixels, multiples of 8) where no table gives it
    int dx, dy, ww, wh;                               // the window inside the cover (dx, dy where no table gives them) and its size
    uint32_t mirror;                                  // where no table gives it
};
template <int E> struct YkNormElem;
template <> struct YkNormElem<YK_ELEM_F16> { typedef _Float16 T; };
template <> struct YkNormElem<YK_ELEM_BF16> { typedef __bf16 T; };
template <> struct YkNormElem<YK_ELEM_F32> { typedef float T; };

template <class T>
__device__ __forceinline__ T yk_dn_value(uint32_t word, int byte, float scale, float bias) {
#pragma clang fp contract(off)
    const float v = (float)((word >> (8 * byte)) & 255u);
    const float m = v * scale;
    const float f = m + bias;
    return (T)f;
}
// a whole row segment (lo, hi: the dwords of each plane, already reversed if mirrored) -> 8 pixels from o on
template <class T, int C, bool PLANAR>
__device__ __forceinline__ void yk_dn_emit(uint8_t* o, size_t planeBytes, const YkDetileNorm& nm, const uint32_t (&lo)[4], const uint32_t (&hi)[4]) {
    if constexpr (PLANAR) {
#pragma unroll
        for (int k = 0; k < C; k++) {
            T e[8];
#pragma unroll
            for (int i = 0; i < 8; i++) e[i] = yk_dn_value<T>(i < 4 ? lo[k] : hi[k], i & 3, nm.scale[k], nm.bias[k]);
            __builtin_memcpy(o + (size_t)k * planeBytes, e, sizeof(e));
        }
    } else {
        T e[8 * C];
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < C; k++) e[i * C + k] = yk_dn_value<T>(i < 4 ? lo[k] : hi[k], i & 3, nm.scale[k], nm.bias[k]);
        __builtin_memcpy(o, e, sizeof(e));
    }
}
// columns src0 .. src0 + n - 1 (n < 8) of a row segment -> n pixels from o on, a predicated store (or C of them, CHW) per pixel
template <class T, int C, bool PLANAR>
__device__ __forceinline__ void yk_dn_emit_px(uint8_t* o, size_t planeBytes, const YkDetileNorm& nm, int src0, int n, const uint32_t (&lo)[4], const uint32_t (&hi)[4]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (i < src0 || i >= src0 + n) continue;
        T e[C];
#pragma unroll
        for (int k = 0; k < C; k++) e[k] = yk_dn_value<T>(i < 4 ? lo[k] : hi[k], i & 3, nm.scale[k], nm.bias[k]);
        if constexpr (PLANAR) {
#pragma unroll
            for (int k = 0; k < C; k++) __builtin_memcpy(o + (size_t)k * planeBytes + (size_t)(i - src0) * sizeof(T), &e[k], sizeof(T));
        } else {
            __builtin_memcpy(o + (size_t)(i - src0) * (C * sizeof(T)), e, sizeof(e));
        }
    }
}
// the two rows of cover tile (jx, jy) this lane holds, clipped against the window, mirrored if asked, converted
template <int E, int C, bool PLANAR, int ASRC>
__device__ __forceinline__ void yk_dn_store(const YkDetileArgs& a, const YkDetileNorm& nm, const YkDtUnit& u, uint32_t jx, uint32_t jy, uint32_t rp) {
    typedef typename YkNormElem<E>::T T;
    const YkPxMirrorClip kx = yk_wpx_clip_mirror((int)jx, nm.dx, nm.ww, (int)nm.mirror);
    const YkPxClip ky = yk_wpx_clip((int)jy, nm.dy, nm.wh);
    if (kx.n == 0 || ky.n == 0) return;
    const int src0 = yk_wpx_mirror_src0(kx, (int)nm.mirror);
    uint32_t al[4];
#pragma unroll
    for (int i = 0; i < 4; i++) al[i] = ASRC == YK_DT_ALPHA_PLANE ? u.a[i] : a.alphaConst;
    const uint32_t pl[4][4] = { { u.r.x, u.r.y, u.r.z, u.r.w }, { u.g.x, u.g.y, u.g.z, u.g.w }, { u.b.x, u.b.y, u.b.z, u.b.w }, { al[0], al[1], al[2], al[3] } };
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int row = (int)rp * 2 + i;                                      // of the tile
        if (row < ky.src0 || row >= ky.src0 + ky.n) continue;
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t l = pl[k][2 * i], h = pl[k][2 * i + 1];
            lo[k] = nm.mirror ? __builtin_bswap32(h) : l;
            hi[k] = nm.mirror ? __builtin_bswap32(l) : h;
        }
        uint8_t* o = a.out + (size_t)(ky.dst + row - ky.src0) * a.rowBytes + (size_t)kx.dst * ((PLANAR ? 1 : C) * sizeof(T));
        if (kx.n == 8) yk_dn_emit<T, C, PLANAR>(o, a.planeBytes, nm, lo, hi);
        else yk_dn_emit_px<T, C, PLANAR>(o, a.planeBytes, nm, src0, kx.n, lo, hi);
    }
}
// frame blockIdx.y of nFrames: its cover from wins[f] (or nm.cx0, nm.cy0), the window's offset inside it from off[2f], off[2f + 1] (or nm.dx, nm.dy),
// its mirror flag from mirror[f] (or nm.mirror); a.nTiles = the cover's wtW x wtH tiles; a.alpha (YK_DT_ALPHA_PLANE) is frame 0's whole plane
template <int E, int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_norm_kernel(YkDetileArgs a, YkDetileNorm nm, const DWinRect* __restrict__ wins, const int* __restrict__ off,
                                                                           const uint32_t* __restrict__ mirror, uint32_t wtW, size_t planesFrame, size_t outFrame,
                                                                           size_t alphaFrame) {
    const uint32_t f = blockIdx.y;
    if (wins) { nm.cx0 = (uint32_t)wins[f].x0; nm.cy0 = (uint32_t)wins[f].y0; }
    if (off) { nm.dx = off[2 * f]; nm.dy = off[2 * f + 1]; }
    if (mirror) nm.mirror = mirror[f];
    a.planes += (size_t)f * planesFrame; a.out += (size_t)f * outFrame;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) a.alpha += (size_t)f * alphaFrame + (size_t)nm.cy0 * a.strideA + nm.cx0;
    const YkDetileWin wn = { nm.cx0 >> 3, nm.cy0 >> 3, wtW };
    const uint32_t bx = blockIdx.x, lane = threadIdx.x & 63, rp = lane & 3;
    const uint32_t j0 = (bx * (YK_DT_K * 4) + (threadIdx.x >> 6)) * 16 + (lane >> 2);
    if ((bx + 1) * (uint32_t)YK_DT_TILES <= a.nTiles) {
        YkDtUnit u[YK_DT_K];                                                  // every unit of the workgroup exists: all loads first
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) yk_dt_load_win<C, PLANAR, ASRC>(a, wn, j0 + k * 64, rp, u[k]);
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) {
            const uint32_t j = j0 + k * 64, jy = j / wn.wtW;
            yk_dn_store<E, C, PLANAR, ASRC>(a, nm, u[k], j - jy * wn.wtW, jy, rp);
        }
        return;
    }
    for (int k = 0; k < YK_DT_K; k++) {
        const uint32_t j = j0 + k * 64, jy = j / wn.wtW;
        if (j >= a.nTiles) continue;
        YkDtUnit u;
        yk_dt_load_win<C, PLANAR, ASRC>(a, wn, j, rp, u);
        yk_dn_store<E, C, PLANAR, ASRC>(a, nm, u, j - jy * wn.wtW, jy, rp);
    }
}
template <int E>
static void yk_dn_launch(const YkDetileArgs& a, const YkDetileNorm& nm, hipStream_t s, int channels, bool planar, bool fromPlane, int nFrames, const DWinRect* wins,
                         const int* off, const uint32_t* mirror, uint32_t wtW, size_t planesFrame, size_t outFrame, size_t alphaFrame) {
    const unsigned gx = (a.nTiles + YK_DT_TILES - 1) / YK_DT_TILES;
    yk_dt_each(channels, planar, fromPlane, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((yk_dec_detile_norm_kernel<E, T::c, T::planar, T::asrc>), dim3(gx, (unsigned)nFrames), dim3(YK_DT_THREADS), 0, s, a, nm, wins, off, mirror, wtW,
                           planesFrame, outFrame, alphaFrame);
    });
}

// ---- the resampling output: a rectangle per frame, bilinear in 16.16 fixed point, to one ow x oh (yk_decode_output_resampled_*) ------
// Not a de-tile: the lanes enumerate OUTPUT pixels and gather their four taps from the 8x8-tiled planes (tap (X, Y) of a colour plane is byte
// ((Y >> 3) * tileW + (X >> 3)) * 64 + (Y & 7) * 8 + (X & 7); alpha taps come from the linear 'ALPM' plane).  The arithmetic is yk_resample.h's,
// the same functions the CPU tool checks.  Frame blockIdx.y reads its nine words {x0, y0, sw - 1, sh - 1, stepX, offX, stepY, offY, mirror} through
// a uniform address (scalar loads).  A workgroup owns 64 x 16 output pixels, so its source footprint is one compact patch that stays in L1 / L2; a
// lane owns four consecutive output columns of one row: it issues every tap load (2 rows x 2 taps x 4 columns per plane, byte loads) before the
// first blend, and stores 4 C elements (HWC) or 4 elements per plane (CHW) through byte pointers like yk_dt_emit, so one path serves every base and
// pitch.  Mirror is applied to the output: the lane's destination column d reads output index ow - 1 - d, and the stores stay rising.  The float
// elements are yk_dn_value's (contraction off: two roundings).  No LDS, no barrier; a lane past the right or bottom edge leaves at once.
#define YK_RS_BW 64                                 // output columns per workgroup: 16 lanes x 4
#define YK_RS_BH 16                                 // output rows per workgroup
struct YkResampleArgs {
    const uint8_t* planes; size_t planeSize, planesFrame;
    const uint8_t* alpha; size_t strideA, alphaFrame;   // YK_DT_ALPHA_PLANE: frame 0's whole plane
    uint32_t alphaConst;                                // YK_DT_ALPHA_CONST: the byte (a constant resamples to itself)
    uint8_t* out; size_t rowBytes, planeBytes, outFrame;
    uint32_t tileW, nbx; int ow, oh;
    float scale[4], bias[4];
    const int* tab;                                     // YK_RS_WORDS per frame
};
template <int E> struct YkRsElem { typedef typename YkNormElem<E>::T T; };
template <> struct YkRsElem<0> { typedef uint8_t T; };
template <class T>
__device__ __forceinline__ T yk_rs_value(uint32_t v, float scale, float bias) {
    if constexpr (sizeof(T) == 1) return (T)v;
    else return yk_dn_value<T>(v, 0, scale, bias);
}
template <int E, int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(256) void yk_dec_resample_kernel(const YkResampleArgs a) {
    typedef typename YkRsElem<E>::T T;
    const uint32_t f = blockIdx.y;
    const int* __restrict__ t = a.tab + (size_t)f * YK_RS_WORDS;
    const int x0 = t[0], y0 = t[1], sw = t[2] + 1, sh = t[3] + 1, mirror = t[8];
    const YkRsAxis ax = { t[4], t[5] }, ay = { t[6], t[7] };
    const uint32_t by = blockIdx.x / a.nbx, bx = blockIdx.x - by * a.nbx;
    const int oy = (int)(by * YK_RS_BH + (threadIdx.x >> 4)), d0 = (int)((bx * 16 + (threadIdx.x & 15)) * 4);
    if (oy >= a.oh || d0 >= a.ow) return;
    const int nk = a.ow - d0 < 4 ? a.ow - d0 : 4;
    const YkRsTap ty = yk_rs_tap(ay, oy, sh);
    const uint32_t Y0 = (uint32_t)(y0 + ty.i0), Y1 = (uint32_t)(y0 + ty.i1);
    const size_t r0 = (size_t)(Y0 >> 3) * a.tileW * 64 + (Y0 & 7) * 8, r1 = (size_t)(Y1 >> 3) * a.tileW * 64 + (Y1 & 7) * 8;
    uint32_t X0[4], X1[4]; int fx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int d = d0 + (k < nk ? k : nk - 1);                              // a column past the edge repeats the last one: its loads stay inside, nothing is stored
        const YkRsTap tx = yk_rs_tap(ax, mirror ? a.ow - 1 - d : d, sw);
        X0[k] = (uint32_t)(x0 + tx.i0); X1[k] = (uint32_t)(x0 + tx.i1); fx[k] = tx.f;
    }
    constexpr int NP = ASRC == YK_DT_ALPHA_PLANE ? 4 : 3;                     // planes that are loaded
    const uint8_t* const P = a.planes + (size_t)f * a.planesFrame;
    uint32_t s[NP][4][4];                                                     // [plane][column][a b c d]: every load before the arithmetic
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const uint8_t* const pl = P + (size_t)p * a.planeSize;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t ca = (X0[k] >> 3) * 64 + (X0[k] & 7), cb = (X1[k] >> 3) * 64 + (X1[k] & 7);
            s[p][k][0] = pl[r0 + ca]; s[p][k][1] = pl[r0 + cb]; s[p][k][2] = pl[r1 + ca]; s[p][k][3] = pl[r1 + cb];
        }
    }
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) {
        const uint8_t* const A = a.alpha + (size_t)f * a.alphaFrame;
        const size_t q0 = (size_t)Y0 * a.strideA, q1 = (size_t)Y1 * a.strideA;
#pragma unroll
        for (int k = 0; k < 4; k++) { s[3][k][0] = A[q0 + X0[k]]; s[3][k][1] = A[q0 + X1[k]]; s[3][k][2] = A[q1 + X0[k]]; s[3][k][3] = A[q1 + X1[k]]; }
    }
    T e[4][C];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int p = 0; p < C; p++) {
            const uint32_t v = p < NP ? (uint32_t)yk_rs_blend((int)s[p < NP ? p : 0][k][0], (int)s[p < NP ? p : 0][k][1], (int)s[p < NP ? p : 0][k][2], (int)s[p < NP ? p : 0][k][3], fx[k], ty.f)
                                      : a.alphaConst;
            e[k][p] = yk_rs_value<T>(v, a.scale[p], a.bias[p]);
        }
    uint8_t* const o = a.out + (size_t)f * a.outFrame + (size_t)oy * a.rowBytes + (size_t)d0 * ((PLANAR ? 1 : C) * sizeof(T));
    if (nk == 4) {
        if constexpr (PLANAR) {
#pragma unroll
            for (int p = 0; p < C; p++) {
                T q[4];
#pragma unroll
                for (int k = 0; k < 4; k++) q[k] = e[k][p];
                __builtin_memcpy(o + (size_t)p * a.planeBytes, q, sizeof(q));
            }
        } else __builtin_memcpy(o, e, sizeof(e));
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (k >= nk) break;
        if constexpr (PLANAR) {
#pragma unroll
            for (int p = 0; p < C; p++) __builtin_memcpy(o + (size_t)p * a.planeBytes + (size_t)k * sizeof(T), &e[k][p], sizeof(T));
        } else __builtin_memcpy(o + (size_t)k * (C * sizeof(T)), e[k], sizeof(e[k]));
    }
}
template <int E>
static void yk_rs_launch(const YkResampleArgs& a, hipStream_t s, int channels, bool planar, bool fromPlane, int nFrames) {
    const unsigned nby = ((unsigned)a.oh + YK_RS_BH - 1) / YK_RS_BH;
    yk_dt_each(channels, planar, fromPlane, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((yk_dec_resample_kernel<E, T::c, T::planar, T::asrc>), dim3(a.nbx * nby, (unsigned)nFrames), dim3(256), 0, s, a);
    });
}

// nFrames == 0: the selected frame (the existing single-image launch); otherwise nFrames frames, planesFrame / outFrame bytes apart
template <int C, bool PLANAR, int ASRC>
static void yk_dt_launch(const YkDetileArgs& a, hipStream_t s, int nFrames = 0, size_t planesFrame = 0, size_t outFrame = 0, size_t alphaFrame = 0,
                         const YkDetileWin* wn = nullptr) {
    const unsigned gx = (a.nTiles + YK_DT_TILES - 1) / YK_DT_TILES;
    if (wn) { hipLaunchKernelGGL((yk_dec_detile_win_kernel<C, PLANAR, ASRC>), dim3(gx), dim3(YK_DT_THREADS), 0, s, a, *wn); return; }
    if (nFrames) { hipLaunchKernelGGL((yk_dec_detile_batch_kernel<C, PLANAR, ASRC>), dim3(gx, (unsigned)nFrames), dim3(YK_DT_THREADS), 0, s, a, planesFrame, outFrame, alphaFrame); return; }
    hipLaunchKernelGGL((yk_dec_detile_kernel<C, PLANAR, ASRC>), dim3(gx), dim3(YK_DT_THREADS), 0, s, a);
}

// the de-tile of the image begun on c into out; alpha: a plane (strideA bytes per row) or NULL with alphaConst 0..255 (channels 4)
// frameBytes / nFrames: every frame of a batch in one launch, frame f at out + f * frameBytes, its alpha plane (if any) at alpha + f * alphaFrame;
// nFrames == 0: the selected frame
// window: the window set on c (yk_decode_set_window) into a ww x wh destination, alpha read at the window's offset (single image only)
static int yk_dec_detile(yk_ctx* c, uint8_t* out, size_t rowBytes, size_t planeBytes, int channels, const uint8_t* alpha, size_t strideA, int alphaConst,
                         int nFrames = 0, size_t frameBytes = 0, size_t alphaFrame = 0, bool window = false) {
    YkDetileArgs a;
    a.planes = yk_dec_frame(c, nFrames ? 0 : c->dCur).planes; a.planeSize = c->dPlaneSize;
    const size_t pf = c->dStride.planes;
    a.alpha = alpha; a.strideA = strideA; a.alphaConst = (uint32_t)(alphaConst & 255) * 0x01010101u;
    a.out = out; a.rowBytes = rowBytes; a.planeBytes = planeBytes;
    a.tileW = (uint32_t)(c->dw >> 3); a.nTiles = (uint32_t)(c->dw >> 3) * (uint32_t)(c->dh >> 3);
    const YkDetileWin win = { (uint32_t)(c->dWinX >> 3), (uint32_t)(c->dWinY >> 3), (uint32_t)(c->dWinW >> 3) };
    const YkDetileWin* wn = window ? &win : nullptr;
    if (window) {
        a.nTiles = (uint32_t)(c->dWinW >> 3) * (uint32_t)(c->dWinH >> 3);
        if (alpha) a.alpha = alpha + (size_t)c->dWinY * strideA + (size_t)c->dWinX;
    }
    const bool planar = planeBytes > 0;
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_DETILE); if (rc) return rc; }
    if (window && c->dPxSet && !yk_wpx_aligned(c->dPxX, c->dPxY, c->dPxW, c->dPxH)) {   // the cover's tiles, clipped to the pixel window (an aligned one is its own cover)
        const YkDetileClip cl = { c->dPxX - c->dWinX, c->dPxY - c->dWinY, c->dPxW, c->dPxH };
        const unsigned gx = (a.nTiles + YK_DT_TILES - 1) / YK_DT_TILES;
        yk_dt_each(channels, planar, alpha != nullptr, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((yk_dec_detile_win_px_kernel<T::c, T::planar, T::asrc>), dim3(gx), dim3(YK_DT_THREADS), 0, c->stream, a, win, cl);
        });
        YK_HIP(c, hipGetLastError());
        return yk_stage_end(c, YK_STAGE_DEC_DETILE);
    }
    if (channels == 3) { if (planar) yk_dt_launch<3, true, YK_DT_ALPHA_NONE>(a, c->stream, nFrames, pf, frameBytes, 0, wn); else yk_dt_launch<3, false, YK_DT_ALPHA_NONE>(a, c->stream, nFrames, pf, frameBytes, 0, wn); }
    else if (alpha)    { if (planar) yk_dt_launch<4, true, YK_DT_ALPHA_PLANE>(a, c->stream, nFrames, pf, frameBytes, alphaFrame, wn); else yk_dt_launch<4, false, YK_DT_ALPHA_PLANE>(a, c->stream, nFrames, pf, frameBytes, alphaFrame, wn); }
    else               { if (planar) yk_dt_launch<4, true, YK_DT_ALPHA_CONST>(a, c->stream, nFrames, pf, frameBytes, 0, wn); else yk_dt_launch<4, false, YK_DT_ALPHA_CONST>(a, c->stream, nFrames, pf, frameBytes, 0, wn); }
    YK_HIP(c, hipGetLastError());
    return yk_stage_end(c, YK_STAGE_DEC_DETILE);
}

// ---- the de-tile at reduced resolution (yk_decode_output_scaled_device and its kin) ---------------------------------------------
// LEVEL 1, 2, 3: s = 1 << LEVEL, out[Y][X][k] = (sum of the s x s box of the whole decode at (s X, s Y) + s s / 2) >> (2 LEVEL), straight from the
// level-0 bytes.  A box never crosses an 8x8 tile, so the lanes that hold a tile's bytes reduce them: the loads, the lane mapping, the units and
// the steps are those of the kernels above (a lane owns the row pair rp of a tile, four lanes a tile, all loads of a workgroup before its first
// store); only what is stored differs.  Sums stay packed: a dword holds two 16-bit sums (the largest, 64 * 255, fits), rounded once at the end.
//   LEVEL 1: the row pair is one output row of 4 pixels; every lane stores, at row 4 ty + rp.
//   LEVEL 2: the row pair gives the upper or lower half of 2 pixels; lanes rp ^ 1 exchange halves (DPP quad_perm, no LDS), the even lane stores
//            at row 2 ty + rp / 2.
//   LEVEL 3: the 16 bytes of the lane are summed (v_sad_u8), lanes rp ^ 1 and then rp ^ 2 add up, lane rp == 0 stores the tile's pixel.
// The four lanes of a tile share its index, so a quad is active or idle as a whole on the last-workgroup path and the exchanges read live lanes.
// Adjacent tiles of a wave write adjacent bytes of an output row, as above.  The alpha plane (linear, two 8-byte rows per lane) has the shape
// of a lane's plane bytes and takes the same reduction.
__device__ __forceinline__ uint32_t yk_dts_quad_xor1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true); }   // quad_perm [1, 0, 3, 2]
__device__ __forceinline__ uint32_t yk_dts_quad_xor2(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true); }   // quad_perm [2, 3, 0, 1]
// the two 2x2 box sums of 4 columns of a row pair, as 16-bit halves (each <= 1020)
__device__ __forceinline__ uint32_t yk_dts_pairs(uint32_t top, uint32_t bot) {
    const uint32_t m = 0x00ff00ffu;
    return (top & m) + ((top >> 8) & m) + (bot & m) + ((bot >> 8) & m);
}
// a lane's 16 bytes of one plane (.x .y = row 0, .z .w = row 1) -> the 4 >> (LEVEL - 1) pixels its quad owes for them, pixel p in byte p
// (LEVEL 2: valid in both lanes of a pair; LEVEL 3: in all four)
template <int LEVEL>
__device__ __forceinline__ uint32_t yk_dts_reduce(const yk_dt4 p) {
    if constexpr (LEVEL == 1) {
        const uint32_t lo = ((yk_dts_pairs(p.x, p.z) + 0x00020002u) >> 2) & 0x00ff00ffu;          // pixels 0, 1 in bytes 0, 2
        const uint32_t hi = ((yk_dts_pairs(p.y, p.w) + 0x00020002u) >> 2) & 0x00ff00ffu;          // pixels 2, 3
        return __builtin_amdgcn_perm(hi, lo, 0x06040200u);
    } else if constexpr (LEVEL == 2) {
        // 2 rows x 4 columns: the left box in the low half, the right box in the high half (each <= 2040, <= 4080 with the other lane's)
        uint32_t t = __builtin_amdgcn_sad_u8(p.x, 0u, __builtin_amdgcn_sad_u8(p.z, 0u, 0u)) | (__builtin_amdgcn_sad_u8(p.y, 0u, __builtin_amdgcn_sad_u8(p.w, 0u, 0u)) << 16);
        t += yk_dts_quad_xor1(t);
        t = ((t + 0x00080008u) >> 4) & 0x00ff00ffu;
        return __builtin_amdgcn_perm(0u, t, 0x0c0c0200u);
    } else {
        uint32_t s = __builtin_amdgcn_sad_u8(p.x, 0u, __builtin_amdgcn_sad_u8(p.y, 0u, __builtin_amdgcn_sad_u8(p.z, 0u, __builtin_amdgcn_sad_u8(p.w, 0u, 0u))));
        s += yk_dts_quad_xor1(s);
        s += yk_dts_quad_xor2(s);                                                                  // <= 64 * 255
        return (s + 32u) >> 6;
    }
}
// NP = 4 >> (LEVEL - 1) pixels of an output row (pixel p of a channel in byte p of its dword) -> their bytes at o (HWC) or o + k * planeBytes (CHW)
template <int C, bool PLANAR, int LEVEL>
__device__ __forceinline__ void yk_dts_emit(uint8_t* o, size_t planeBytes, uint32_t r, uint32_t g, uint32_t b, uint32_t al) {
    constexpr int NP = 4 >> (LEVEL - 1);
    if constexpr (PLANAR) {
        const uint32_t v[4] = { r, g, b, al };
#pragma unroll
        for (int k = 0; k < C; k++) __builtin_memcpy(o + (size_t)k * planeBytes, &v[k], NP);
    } else if constexpr (LEVEL == 1 && C == 3) {
        const uint32_t rg0 = __builtin_amdgcn_perm(g, r, 0x05010400u), rg1 = __builtin_amdgcn_perm(g, r, 0x07030602u);
        const uint32_t wd[3] = { __builtin_amdgcn_perm(b, rg0, 0x02040100u), __builtin_amdgcn_perm(rg1, __builtin_amdgcn_perm(b, g, 0x05010400u), 0x05040302u),
                                 __builtin_amdgcn_perm(b, rg1, 0x07030206u) };
        __builtin_memcpy(o, wd, 12);
    } else if constexpr (LEVEL == 1) {
        const uint32_t rgL = __builtin_amdgcn_perm(g, r, 0x05010400u), rgH = __builtin_amdgcn_perm(g, r, 0x07030602u);
        const uint32_t baL = __builtin_amdgcn_perm(al, b, 0x05010400u), baH = __builtin_amdgcn_perm(al, b, 0x07030602u);
        const yk_dt4 px = { __builtin_amdgcn_perm(baL, rgL, 0x05040100u), __builtin_amdgcn_perm(baL, rgL, 0x07060302u),
                            __builtin_amdgcn_perm(baH, rgH, 0x05040100u), __builtin_amdgcn_perm(baH, rgH, 0x07060302u) };
        __builtin_memcpy(o, &px, 16);
    } else {
        const uint32_t rg = __builtin_amdgcn_perm(g, r, 0x05010400u);                              // r0 g0 r1 g1
        if constexpr (C == 3) {
            const uint32_t wd[2] = { __builtin_amdgcn_perm(b, rg, 0x02040100u), __builtin_amdgcn_perm(b, rg, 0x0c0c0503u) };   // r0 g0 b0 r1 | g1 b1
            __builtin_memcpy(o, wd, 3 * NP);
        } else {
            const uint32_t ba = __builtin_amdgcn_perm(al, b, 0x05010400u);                         // b0 a0 b1 a1
            const uint32_t wd[2] = { __builtin_amdgcn_perm(ba, rg, 0x05040100u), __builtin_amdgcn_perm(ba, rg, 0x07060302u) };
            __builtin_memcpy(o, wd, 4 * NP);
        }
    }
}

struct YkDtsUnit { yk_dt4 r, g, b, a; size_t o; };

// tile `src` of the planes, whose reduced pixels go to tile position (jx, jy) of the destination; the alpha plane is read at (8 jx, 8 jy)
template <int C, bool PLANAR, int ASRC, int LEVEL>
__device__ __forceinline__ void yk_dts_load(const YkDetileArgs& a, size_t src, uint32_t jx, uint32_t jy, uint32_t rp, YkDtsUnit& u) {
    const size_t ti = src * 64 + rp * 16;
    u.r = *reinterpret_cast<const yk_dt4*>(a.planes + ti);
    u.g = *reinterpret_cast<const yk_dt4*>(a.planes + a.planeSize + ti);
    u.b = *reinterpret_cast<const yk_dt4*>(a.planes + 2 * a.planeSize + ti);
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) {
        const size_t y = (size_t)jy * 8 + rp * 2, x = (size_t)jx * 8;
        uint32_t al[4];
        __builtin_memcpy(&al[0], a.alpha + y * a.strideA + x, 8);
        __builtin_memcpy(&al[2], a.alpha + (y + 1) * a.strideA + x, 8);
        u.a = yk_dt4{ al[0], al[1], al[2], al[3] };
    }
    u.o = ((size_t)jy * (8 >> LEVEL) + (rp >> (LEVEL - 1))) * a.rowBytes + (size_t)jx * (8 >> LEVEL) * (PLANAR ? 1 : C);
}
template <int C, bool PLANAR, int ASRC, int LEVEL>
__device__ __forceinline__ void yk_dts_store(const YkDetileArgs& a, const YkDtsUnit& u, uint32_t rp) {
    const uint32_t r = yk_dts_reduce<LEVEL>(u.r), g = yk_dts_reduce<LEVEL>(u.g), b = yk_dts_reduce<LEVEL>(u.b);
    uint32_t al = a.alphaConst;                                               // a constant is its own mean
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) al = yk_dts_reduce<LEVEL>(u.a);
    if ((rp & ((1u << (LEVEL - 1)) - 1)) == 0) yk_dts_emit<C, PLANAR, LEVEL>(a.out + u.o, a.planeBytes, r, g, b, al);
}
// WIN: the tiles of the window wn, row-major (yk_dt_load_win's addressing); otherwise the image's tiles in plane order
template <int C, bool PLANAR, int ASRC, int LEVEL, bool WIN>
__device__ __forceinline__ void yk_dts_unit(const YkDetileArgs& a, const YkDetileWin& wn, uint32_t j, uint32_t rp, YkDtsUnit& u) {
    const uint32_t rowW = WIN ? wn.wtW : a.tileW;
    const uint32_t jy = j / rowW, jx = j - jy * rowW;
    const size_t src = WIN ? (size_t)(wn.ty0 + jy) * a.tileW + wn.tx0 + jx : (size_t)j;
    yk_dts_load<C, PLANAR, ASRC, LEVEL>(a, src, jx, jy, rp, u);
}
template <int C, bool PLANAR, int ASRC, int LEVEL, bool WIN>
__device__ __forceinline__ void yk_dec_detile_scaled_body(const YkDetileArgs& a, const YkDetileWin& wn, const uint32_t bx) {
    const uint32_t lane = threadIdx.x & 63, rp = lane & 3;
    const uint32_t j0 = (bx * (YK_DT_K * 4) + (threadIdx.x >> 6)) * 16 + (lane >> 2);
    if ((bx + 1) * (uint32_t)YK_DT_TILES <= a.nTiles) {
        YkDtsUnit u[YK_DT_K];                                                 // every unit of the workgroup exists: all loads first
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) yk_dts_unit<C, PLANAR, ASRC, LEVEL, WIN>(a, wn, j0 + k * 64, rp, u[k]);
#pragma unroll
        for (int k = 0; k < YK_DT_K; k++) yk_dts_store<C, PLANAR, ASRC, LEVEL>(a, u[k], rp);
        return;
    }
    for (int k = 0; k < YK_DT_K; k++) {                                       // the last workgroup: tiles up to nTiles, whole quads
        const uint32_t j = j0 + k * 64;
        if (j >= a.nTiles) continue;
        YkDtsUnit u;
        yk_dts_unit<C, PLANAR, ASRC, LEVEL, WIN>(a, wn, j, rp, u);
        yk_dts_store<C, PLANAR, ASRC, LEVEL>(a, u, rp);
    }
}
// the selected frame (gridDim.y == 1, strides unused) or every frame of a batch: frame blockIdx.y as in yk_dec_detile_batch_kernel
template <int C, bool PLANAR, int ASRC, int LEVEL>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_scaled_batch_kernel(YkDetileArgs a, size_t planesFrame, size_t outFrame, size_t alphaFrame) {
    a.planes += (size_t)blockIdx.y * planesFrame; a.out += (size_t)blockIdx.y * outFrame;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) a.alpha += (size_t)blockIdx.y * alphaFrame;
    yk_dec_detile_scaled_body<C, PLANAR, ASRC, LEVEL, false>(a, YkDetileWin{ 0, 0, a.tileW }, blockIdx.x);
}
template <int C, bool PLANAR, int ASRC, int LEVEL>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_scaled_win_kernel(YkDetileArgs a, const YkDetileWin wn) {
    yk_dec_detile_scaled_body<C, PLANAR, ASRC, LEVEL, true>(a, wn, blockIdx.x);
}
// K windows of a prepared image, as in yk_dec_detile_wins_kernel; windowBytes apart at the reduced size
template <int C, bool PLANAR, int ASRC, int LEVEL>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_detile_scaled_wins_kernel(YkDetileArgs a, const int* __restrict__ xy, uint32_t wtW, size_t windowBytes) {
    const uint32_t k = blockIdx.y;
    const uint32_t x0 = (uint32_t)xy[2 * k], y0 = (uint32_t)xy[2 * k + 1];
    a.out += (size_t)k * windowBytes;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) a.alpha += (size_t)y0 * a.strideA + x0;
    yk_dec_detile_scaled_body<C, PLANAR, ASRC, LEVEL, true>(a, YkDetileWin{ x0 >> 3, y0 >> 3, wtW }, blockIdx.x);
}

// which of the three kernels a scaled de-tile is: K windows from a table (nWindows > 0), the window *wn, or nFrames frames (0: the selected one)
struct YkDtsForm { int nFrames; size_t planesFrame, outFrame, alphaFrame; const YkDetileWin* wn; int nWindows; const int* devXY; uint32_t wtW; size_t windowBytes; };

template <int C, bool PLANAR, int ASRC, int LEVEL>
static void yk_dts_launch_level(const YkDetileArgs& a, hipStream_t s, const YkDtsForm& f) {
    const unsigned gx = (a.nTiles + YK_DT_TILES - 1) / YK_DT_TILES;
    if (f.nWindows) hipLaunchKernelGGL((yk_dec_detile_scaled_wins_kernel<C, PLANAR, ASRC, LEVEL>), dim3(gx, (unsigned)f.nWindows), dim3(YK_DT_THREADS), 0, s, a, f.devXY, f.wtW, f.windowBytes);
    else if (f.wn) hipLaunchKernelGGL((yk_dec_detile_scaled_win_kernel<C, PLANAR, ASRC, LEVEL>), dim3(gx), dim3(YK_DT_THREADS), 0, s, a, *f.wn);
    else hipLaunchKernelGGL((yk_dec_detile_scaled_batch_kernel<C, PLANAR, ASRC, LEVEL>), dim3(gx, (unsigned)(f.nFrames ? f.nFrames : 1)), dim3(YK_DT_THREADS), 0, s, a,
                            f.planesFrame, f.outFrame, f.alphaFrame);
}
template <int C, bool PLANAR, int ASRC>
static void yk_dts_launch(const YkDetileArgs& a, hipStream_t s, const YkDtsForm& f, int level) {
    if (level == 1) yk_dts_launch_level<C, PLANAR, ASRC, 1>(a, s, f);
    else if (level == 2) yk_dts_launch_level<C, PLANAR, ASRC, 2>(a, s, f);
    else yk_dts_launch_level<C, PLANAR, ASRC, 3>(a, s, f);
}
// level 1..3; a: the arguments of the full-size launch (tiles, pitches of the REDUCED destination); one YK_STAGE_DEC_DETILE interval
static int yk_dts_run(yk_ctx* c, const YkDetileArgs& a, const YkDtsForm& f, int level, int channels) {
    const bool planar = a.planeBytes > 0;
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_DETILE); if (rc) return rc; }
    if (channels == 3) { if (planar) yk_dts_launch<3, true, YK_DT_ALPHA_NONE>(a, c->stream, f, level); else yk_dts_launch<3, false, YK_DT_ALPHA_NONE>(a, c->stream, f, level); }
    else if (a.alpha)  { if (planar) yk_dts_launch<4, true, YK_DT_ALPHA_PLANE>(a, c->stream, f, level); else yk_dts_launch<4, false, YK_DT_ALPHA_PLANE>(a, c->stream, f, level); }
    else               { if (planar) yk_dts_launch<4, true, YK_DT_ALPHA_CONST>(a, c->stream, f, level); else yk_dts_launch<4, false, YK_DT_ALPHA_CONST>(a, c->stream, f, level); }
    YK_HIP(c, hipGetLastError());
    return yk_stage_end(c, YK_STAGE_DEC_DETILE);
}
// yk_dec_detile at level 1..3: the same arguments, the destination at the reduced size
static int yk_dec_detile_scaled(yk_ctx* c, int level, uint8_t* out, size_t rowBytes, size_t planeBytes, int channels, const uint8_t* alpha, size_t strideA, int alphaConst,
                                int nFrames = 0, size_t frameBytes = 0, size_t alphaFrame = 0, bool window = false) {
    YkDetileArgs a;
    a.planes = yk_dec_frame(c, nFrames ? 0 : c->dCur).planes; a.planeSize = c->dPlaneSize;
    a.alpha = alpha; a.strideA = strideA; a.alphaConst = (uint32_t)(alphaConst & 255) * 0x01010101u;
    a.out = out; a.rowBytes = rowBytes; a.planeBytes = planeBytes;
    a.tileW = (uint32_t)(c->dw >> 3); a.nTiles = (uint32_t)(c->dw >> 3) * (uint32_t)(c->dh >> 3);
    const YkDetileWin win = { (uint32_t)(c->dWinX >> 3), (uint32_t)(c->dWinY >> 3), (uint32_t)(c->dWinW >> 3) };
    if (window) {
        a.nTiles = (uint32_t)(c->dWinW >> 3) * (uint32_t)(c->dWinH >> 3);
        if (alpha) a.alpha = alpha + (size_t)c->dWinY * strideA + (size_t)c->dWinX;
    }
    const YkDtsForm f = { nFrames, c->dStride.planes, frameBytes, alphaFrame, window ? &win : nullptr, 0, nullptr, 0, 0 };
    return yk_dts_run(c, a, f, level, channels);
}

// ---- the de-tile of a mip chain (yk_decode_output_mipchain[_batch]_device) -------------------------------------------------------
// Level k of a w x h image: out_k[Y][X][c] = (sum of the (1 << k)^2 box of the whole decode at (X << k, Y << k) + (1 << 2k) / 2) >> 2k for
// X < w >> k, Y < h >> k, every level straight from the level-0 bytes.  Two kernels, the planes read once:
//   the block kernel: a workgroup owns one 64x64 block (blockIdx.x = by * nbx + bx, frame blockIdx.y): lane tid holds the row pair tid & 3 of tile
//     tid >> 2 of the block (tile (t & 7, t >> 3)), so a wave loads two tile rows of 512 contiguous bytes per plane with the 16-byte loads of
//     yk_dts_load, and the quads of a tile are those of yk_dts_reduce.  Tiles past the right or bottom edge leave their quads idle.  From its
//     registers a lane stores the levels 0..3 that are asked for (yk_dt_emit, yk_dts_reduce + yk_dts_emit: wave-uniform branches on the
//     destination pointers).  For the levels above, the unrounded sum of a tile (<= 16320) goes to LDS, one dword per lane (lane rp keeps
//     channel rp); wave 0 then holds output o = lane >> 2 (4 x 4 per block), channel lane & 3 of level 4 as the sum of 2x2 tiles and folds it
//     with __shfl_xor to the 2x2 outputs of level 5 and to the block's own sum, which is level 6 and, for the tail, one dword per channel at
//     sums[frame][by][bx][channel].  Every sum is exact in 32 bits (64 * 64 * 255 = 1044480) and is rounded once.  A 16-, 32- or 64-pixel box is
//     stored, and a block sum written, only when it lies wholly inside the image.
//   the tail kernel: a workgroup per output pixel of the levels >= 7 (all of them and every frame in one launch): 64 lanes per channel add the
//     n x n block sums of the box (n = 1 << (k - 6)) in 64 bits, a tree in LDS adds the lanes, the pixel is rounded once.
// A constant alpha is its own mean at every level and is stored as it is.
struct YkMipDst { uint8_t* out; size_t rowBytes, planeBytes, frameBytes; };
struct YkMipArgs {
    const uint8_t* planes; size_t planeSize, planesFrame;
    const uint8_t* alpha; size_t strideA, alphaFrame;        // YK_DT_ALPHA_PLANE
    uint32_t alphaConst;                                      // the byte in all four lanes of a dword
    uint32_t w, h, nbx;                                       // nbx: blocks per block row, the partial one included
    uint32_t high;                                            // a level >= 4 is asked for
    uint32_t* sums; uint32_t sbx, sby;                        // a level >= 7 is asked for: the whole blocks' sums, sbx = w >> 6, sby = h >> 6
    YkMipDst lv[7];                                           // levels 0..6; out == NULL: not asked for
};
struct YkMipTailArgs {
    const uint32_t* sums; uint32_t sbx, sby, w, h, alphaConst;
    int first, last;                                          // levels first..last, 7 <= first
    YkMipDst lv[YK_MIP_MAX_LEVELS - 7];                       // level k at lv[k - 7]
};

// the sum of a tile's 64 bytes of one plane, in all four lanes of its quad
__device__ __forceinline__ uint32_t yk_mip_tile_sum(const yk_dt4 p) {
    uint32_t s = __builtin_amdgcn_sad_u8(p.x, 0u, __builtin_amdgcn_sad_u8(p.y, 0u, __builtin_amdgcn_sad_u8(p.z, 0u, __builtin_amdgcn_sad_u8(p.w, 0u, 0u))));
    s += yk_dts_quad_xor1(s);
    s += yk_dts_quad_xor2(s);
    return s;
}
template <int C, bool PLANAR, int ASRC, int LEVEL>
__device__ __forceinline__ void yk_mip_store_low(const YkMipArgs& a, const YkMipDst& d, const YkDtsUnit& u, uint32_t tx, uint32_t ty, uint32_t rp) {
    const uint32_t r = yk_dts_reduce<LEVEL>(u.r), g = yk_dts_reduce<LEVEL>(u.g), b = yk_dts_reduce<LEVEL>(u.b);
    uint32_t al = a.alphaConst;
    if constexpr (ASRC == YK_DT_ALPHA_PLANE) al = yk_dts_reduce<LEVEL>(u.a);
    const size_t o = (size_t)blockIdx.y * d.frameBytes + ((size_t)ty * (8 >> LEVEL) + (rp >> (LEVEL - 1))) * d.rowBytes + (size_t)tx * (8 >> LEVEL) * (PLANAR ? 1 : C);
    if ((rp & ((1u << (LEVEL - 1)) - 1)) == 0) yk_dts_emit<C, PLANAR, LEVEL>(d.out + o, d.planeBytes, r, g, b, al);
}
// channel ch of pixel (X, Y) of a level
template <int C, bool PLANAR>
__device__ __forceinline__ void yk_mip_store_byte(const YkMipDst& d, uint32_t X, uint32_t Y, uint32_t ch, uint32_t v) {
    uint8_t* o = d.out + (size_t)blockIdx.y * d.frameBytes + (size_t)Y * d.rowBytes;
    if constexpr (PLANAR) o[(size_t)ch * d.planeBytes + X] = (uint8_t)v; else o[(size_t)X * C + ch] = (uint8_t)v;
}

template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(YK_DT_THREADS) void yk_dec_mip_block_kernel(const YkMipArgs a) {
    __shared__ uint32_t tileSum[YK_DT_THREADS];                               // [tile of the block][channel]
    const uint32_t tid = threadIdx.x, rp = tid & 3, t = tid >> 2;
    const uint32_t by = blockIdx.x / a.nbx, bx = blockIdx.x - by * a.nbx;
    const uint32_t tx = bx * 8 + (t & 7), ty = by * 8 + (t >> 3), tileW = a.w >> 3;
    uint32_t mine = 0;
    if (tx < tileW && ty * 8 < a.h) {                                         // whole quads: the four lanes of a tile share t
        YkDtsUnit u;
        const uint8_t* pl = a.planes + (size_t)blockIdx.y * a.planesFrame + ((size_t)ty * tileW + tx) * 64 + rp * 16;
        u.r = *reinterpret_cast<const yk_dt4*>(pl);
        u.g = *reinterpret_cast<const yk_dt4*>(pl + a.planeSize);
        u.b = *reinterpret_cast<const yk_dt4*>(pl + 2 * a.planeSize);
        const size_t y = (size_t)ty * 8 + rp * 2, x = (size_t)tx * 8;
        if constexpr (ASRC == YK_DT_ALPHA_PLANE) {
            const uint8_t* ap = a.alpha + (size_t)blockIdx.y * a.alphaFrame + y * a.strideA + x;
            uint32_t al[4];
            __builtin_memcpy(&al[0], ap, 8);
            __builtin_memcpy(&al[2], ap + a.strideA, 8);
            u.a = yk_dt4{ al[0], al[1], al[2], al[3] };
        } else u.a = yk_dt4{ a.alphaConst, a.alphaConst, a.alphaConst, a.alphaConst };
        if (a.lv[0].out) {
            const YkMipDst& d = a.lv[0];
            uint8_t* o = d.out + (size_t)blockIdx.y * d.frameBytes + y * d.rowBytes + x * (PLANAR ? 1 : C);
            yk_dt_emit<C, PLANAR>(o, d.planeBytes, u.r.x, u.r.y, u.g.x, u.g.y, u.b.x, u.b.y, u.a.x, u.a.y);
            yk_dt_emit<C, PLANAR>(o + d.rowBytes, d.planeBytes, u.r.z, u.r.w, u.g.z, u.g.w, u.b.z, u.b.w, u.a.z, u.a.w);
        }
        if (a.lv[1].out) yk_mip_store_low<C, PLANAR, ASRC, 1>(a, a.lv[1], u, tx, ty, rp);
        if (a.lv[2].out) yk_mip_store_low<C, PLANAR, ASRC, 2>(a, a.lv[2], u, tx, ty, rp);
        if (a.lv[3].out) yk_mip_store_low<C, PLANAR, ASRC, 3>(a, a.lv[3], u, tx, ty, rp);
        if (a.high) {
            const uint32_t sr = yk_mip_tile_sum(u.r), sg = yk_mip_tile_sum(u.g), sb = yk_mip_tile_sum(u.b);
            uint32_t sa = 0;
            if constexpr (ASRC == YK_DT_ALPHA_PLANE) sa = yk_mip_tile_sum(u.a);
            mine = rp == 0 ? sr : rp == 1 ? sg : rp == 2 ? sb : sa;
        }
    }
    if (!a.high) return;
    tileSum[tid] = mine;                                                      // a tile outside the image adds nothing
    __syncthreads();
    if (tid >= 64) return;
    // wave 0: lane = (oy, ox, ch), output (ox, oy) of the block's 4 x 4 at level 4
    const uint32_t ch = tid & 3, ox = (tid >> 2) & 3, oy = tid >> 4;
    const uint32_t t0 = (oy * 16 + ox * 2) * 4 + ch;                          // tile (2 ox, 2 oy)
    const uint32_t s4 = tileSum[t0] + tileSum[t0 + 4] + tileSum[t0 + 32] + tileSum[t0 + 36];
    uint32_t s5 = s4 + (uint32_t)__shfl_xor((int)s4, 4);                      // ox ^ 1
    s5 += (uint32_t)__shfl_xor((int)s5, 16);                                  // oy ^ 1
    uint32_t s6 = s5 + (uint32_t)__shfl_xor((int)s5, 8);                      // ox ^ 2
    s6 += (uint32_t)__shfl_xor((int)s6, 32);                                  // oy ^ 2
    const bool fixed = ch == 3 && ASRC != YK_DT_ALPHA_PLANE;                  // a constant alpha
    const uint32_t ac = a.alphaConst & 255u;
    if (ch < (uint32_t)C) {
        if (a.lv[4].out && bx * 4 + ox < (a.w >> 4) && by * 4 + oy < (a.h >> 4))
            yk_mip_store_byte<C, PLANAR>(a.lv[4], bx * 4 + ox, by * 4 + oy, ch, fixed ? ac : (s4 + 128u) >> 8);
        if (a.lv[5].out && !((ox | oy) & 1) && bx * 2 + (ox >> 1) < (a.w >> 5) && by * 2 + (oy >> 1) < (a.h >> 5))
            yk_mip_store_byte<C, PLANAR>(a.lv[5], bx * 2 + (ox >> 1), by * 2 + (oy >> 1), ch, fixed ? ac : (s5 + 512u) >> 10);
        if (a.lv[6].out && !(ox | oy) && bx < a.sbx && by < a.sby)
            yk_mip_store_byte<C, PLANAR>(a.lv[6], bx, by, ch, fixed ? ac : (s6 + 2048u) >> 12);
    }
    if (a.sums && !(ox | oy) && bx < a.sbx && by < a.sby)
        a.sums[(((size_t)blockIdx.y * a.sby + by) * a.sbx + bx) * 4 + ch] = s6;
}

template <int C, bool PLANAR, int ASRC>
__global__ __launch_bounds__(256) void yk_dec_mip_tail_kernel(const YkMipTailArgs a) {
    __shared__ unsigned long long acc[256];
    uint32_t i = blockIdx.x, Lw = 0;
    int k = a.first;
    for (; k <= a.last; k++) {                                                // the levels' pixels are numbered one level after the other
        Lw = a.w >> k;
        const uint32_t n = Lw * (a.h >> k);
        if (i < n) break;
        i -= n;
    }
    if (k > a.last) return;
    const uint32_t Y = i / Lw, X = i - Y * Lw, sh = (uint32_t)k - 6, n = 1u << sh;
    const uint32_t tid = threadIdx.x, ch = tid & 3;
    const bool fixed = ch == 3 && ASRC != YK_DT_ALPHA_PLANE;
    unsigned long long s = 0;
    if (ch < (uint32_t)C && !fixed) {
        const uint32_t* base = a.sums + (((size_t)blockIdx.y * a.sby + (size_t)Y * n) * a.sbx + (size_t)X * n) * 4 + ch;
        for (uint32_t j = tid >> 2; j < n * n; j += 64) s += base[((size_t)(j >> sh) * a.sbx + (j & (n - 1))) * 4];
    }
    acc[tid] = s;
    __syncthreads();
    for (uint32_t st = 128; st >= 4; st >>= 1) {                              // st is a multiple of 4: a lane adds its own channel
        if (tid < st) acc[tid] += acc[tid + st];
        __syncthreads();
    }
    if (tid < (uint32_t)C) {
        const YkMipDst& d = a.lv[k - 7];
        const uint32_t v = fixed ? (a.alphaConst & 255u) : (uint32_t)((acc[tid] + (1ull << (2 * k - 1))) >> (2 * k));
        yk_mip_store_byte<C, PLANAR>(d, X, Y, ch, v);
    }
}

template <int C, bool PLANAR, int ASRC>
static void yk_mip_launch(const YkMipArgs& a, const YkMipTailArgs& t, hipStream_t s, unsigned nFrames) {
    const unsigned nby = (a.h + 63) >> 6;
    hipLaunchKernelGGL((yk_dec_mip_block_kernel<C, PLANAR, ASRC>), dim3(a.nbx * nby, nFrames), dim3(YK_DT_THREADS), 0, s, a);
    if (t.first > t.last) return;
    unsigned px = 0;
    for (int k = t.first; k <= t.last; k++) px += (t.w >> k) * (t.h >> k);
    hipLaunchKernelGGL((yk_dec_mip_tail_kernel<C, PLANAR, ASRC>), dim3(px, nFrames), dim3(256), 0, s, t);
}

// The reference's RGBA branch as it executes (decoder/YAIK_DefaultCallback.cpp:45-62): the alpha store does not advance dst, so a row is
// w RGB triples followed by ONE alpha byte; the alpha row cursors advance w bytes per tile row instead of 8 * strideA (:36-39 vs
// :128-130), so row y ends on the byte alpha[strideA * (y & 7) + w * (y >> 3) + w - 1].  One thread per row writes that byte.
__global__ __launch_bounds__(256) void yk_dec_ref_alpha_kernel(const uint8_t* __restrict__ alpha, int strideA, size_t alphaBytes, int w, int h,
                                                               uint8_t* __restrict__ out, size_t pitch) {
    const int y = blockIdx.x * 256 + threadIdx.x;
    if (y >= h) return;
    const size_t src = (size_t)strideA * (y & 7) + (size_t)w * (y >> 3) + (size_t)(w - 1);
    out[(size_t)y * pitch + (size_t)w * 3] = src < alphaBytes ? alpha[src] : 0;
}

// ---- host side ---------------------------------------------------------------------------------------------------
static int yk_dec_scratch(yk_ctx* c, size_t bytes) { YK_HIP(c, c->dScratch.reserve(c->stream, bytes)); return YK_OK; }

extern "C" {

// zero every 4x4 cell tile4x4Mask does not mark (thread = 8x8 tile and plane; the mask is shared by the planes until a plane-subset pass splits it)
__device__ __forceinline__ void yk_dec_zero_unmarked_tile(const uint8_t* __restrict__ tile4, size_t tile4Size, int split, int stride4, int tilesW, const size_t i,
                                                          uint8_t* __restrict__ planes, size_t planeSize) {
    const int p = blockIdx.y;
    const int tx = (int)(i % (size_t)tilesW), ty = (int)(i / (size_t)tilesW);
    const uint8_t m = tile4[(split ? (size_t)p * tile4Size : 0) + (size_t)(tx >> 1) + (size_t)ty * stride4];     // byte = 16x8 pixels: bit ((cx>>1)&1)*4 + (cy&1)*2 + (cx&1)
    const int sh = (tx & 1) * 4;
    uint8_t* o = planes + (size_t)p * planeSize + i * 64;
#pragma unroll
    for (int qy = 0; qy < 2; qy++)
#pragma unroll
        for (int qx = 0; qx < 2; qx++)
            if (!((m >> (sh + qy * 2 + qx)) & 1))
                for (int r = 0; r < 4; r++) *reinterpret_cast<uint32_t*>(o + (qy * 4 + r) * 8 + qx * 4) = 0u;
}
__device__ __forceinline__ void yk_dec_zero_unmarked_body(const uint8_t* __restrict__ tile4, size_t tile4Size, int split, int stride4, int tilesW, size_t T8,
                                                          uint8_t* __restrict__ planes, size_t planeSize) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T8) yk_dec_zero_unmarked_tile(tile4, tile4Size, split, stride4, tilesW, i, planes, planeSize);
}
// under a decode window: the window's tiles only (thread j of nWin = window tile (j % wtW, j / wtW)); outside it the planes are nobody's to read
__global__ __launch_bounds__(256) void yk_dec_zero_unmarked_win_kernel(const uint8_t* __restrict__ tile4, size_t tile4Size, int split, int stride4, int tilesW,
                                                                       uint32_t tx0, uint32_t ty0, uint32_t wtW, uint32_t nWin, uint8_t* __restrict__ planes, size_t planeSize) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nWin) return;
    const uint32_t jy = j / wtW, jx = j - jy * wtW;
    yk_dec_zero_unmarked_tile(tile4, tile4Size, split, stride4, tilesW, (size_t)(ty0 + jy) * tilesW + tx0 + jx, planes, planeSize);
}
// a prepared image without a 1-D chunk: the tiles of the blocks of a list, enumerated as yk_dec1d_list_kernel does (nTiles = 64 x the list's length)
__global__ __launch_bounds__(256) void yk_dec_zero_unmarked_list_kernel(const uint8_t* __restrict__ tile4, size_t tile4Size, int stride4, int tilesW, int tilesH,
                                                                        const uint32_t* __restrict__ list, uint32_t xB64, uint32_t nTiles, uint8_t* __restrict__ planes, size_t planeSize) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nTiles) return;
    const uint32_t b = list[j >> 6], t = j & 63u;
    const uint32_t by = b / xB64, tx = (b - by * xB64) * 8u + (t & 7u), ty = by * 8u + (t >> 3);
    if (tx >= (uint32_t)tilesW || ty >= (uint32_t)tilesH) return;
    yk_dec_zero_unmarked_tile(tile4, tile4Size, 0, stride4, tilesW, (size_t)ty * tilesW + tx, planes, planeSize);
}
__global__ __launch_bounds__(256) void yk_dec_zero_unmarked_kernel(const uint8_t* __restrict__ tile4, size_t tile4Size, int split, int stride4, int tilesW, size_t T8,
                                                                   uint8_t* __restrict__ planes, size_t planeSize) {
    yk_dec_zero_unmarked_body(tile4, tile4Size, split, stride4, tilesW, T8, planes, planeSize);
}
// every frame of a batch: frame = blockIdx.z (the masks of a batch are never split)
__global__ __launch_bounds__(256) void yk_dec_zero_unmarked_batch_kernel(const uint8_t* __restrict__ tile4, size_t sTile4, size_t tile4Size, int stride4, int tilesW, size_t T8,
                                                                         uint8_t* __restrict__ planes, size_t sPlanes, size_t planeSize) {
    yk_dec_zero_unmarked_body(tile4 + (size_t)blockIdx.z * sTile4, tile4Size, 0, stride4, tilesW, T8, planes + (size_t)blockIdx.z * sPlanes, planeSize);
}
// a batch with a window per frame: frame = blockIdx.z, the tiles of its window only (thread j of nWin as in the window form above)
__global__ __launch_bounds__(256) void yk_dec_zero_unmarked_batch_win_kernel(const uint8_t* __restrict__ tile4, size_t sTile4, size_t tile4Size, int stride4, int tilesW,
                                                                             const DWinRect* __restrict__ wins, uint32_t wtW, uint32_t nWin, uint8_t* __restrict__ planes,
                                                                             size_t sPlanes, size_t planeSize) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nWin) return;
    const size_t f = blockIdx.z;
    const uint32_t tx0 = (uint32_t)wins[f].x0 >> 3, ty0 = (uint32_t)wins[f].y0 >> 3;
    const uint32_t jy = j / wtW, jx = j - jy * wtW;
    yk_dec_zero_unmarked_tile(tile4 + f * sTile4, tile4Size, 0, stride4, tilesW, (size_t)(ty0 + jy) * tilesW + tx0 + jx, planes + f * sPlanes, planeSize);
}
// a batch with a rectangle per frame (yk_decode_set_batch_rects): the tiles of frame f's own cover; the grid is the largest cover's
__global__ __launch_bounds__(256) void yk_dec_zero_unmarked_batch_rects_kernel(const uint8_t* __restrict__ tile4, size_t sTile4, size_t tile4Size, int stride4, int tilesW,
                                                                               const DWinRect* __restrict__ wins, uint8_t* __restrict__ planes, size_t sPlanes, size_t planeSize) {
    const size_t f = blockIdx.z;
    const DWinRect wr = wins[f];
    const uint32_t wtW = (uint32_t)(wr.x1 - wr.x0) >> 3, nWin = wtW * ((uint32_t)(wr.y1 - wr.y0) >> 3);
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nWin) return;
    const uint32_t jy = j / wtW, jx = j - jy * wtW;
    yk_dec_zero_unmarked_tile(tile4 + f * sTile4, tile4Size, 0, stride4, tilesW, (size_t)(((uint32_t)wr.y0 >> 3) + jy) * tilesW + ((uint32_t)wr.x0 >> 3) + jx, planes + f * sPlanes,
                              planeSize);
}
static int yk_dec_settle(yk_ctx* c) {
    if (!c->dPlanesStale) return YK_OK;
    const int w = c->dw, h = c->dh;
    const size_t T8 = (size_t)(w >> 3) * (h >> 3);
    if (c->dBRectSet) {                                                         // every frame of the batch inside its rectangle's own cover
        hipLaunchKernelGGL(yk_dec_zero_unmarked_batch_rects_kernel, dim3((c->dBRectMaxTiles + 255) / 256, 3, (unsigned)c->dFrames), dim3(256), 0, c->stream, c->dB.tile4,
                           c->dStride.tile4, c->dTile4Size, (w + 15) >> 4, w >> 3, reinterpret_cast<const DWinRect*>(c->dBWinTab.p), c->dB.planes, c->dStride.planes, c->dPlaneSize);
    } else if (c->dBWinSet) {                                                        // every frame of the batch inside its own window
        const uint32_t wtW = (uint32_t)(c->dBWinW >> 3), nWin = wtW * (uint32_t)(c->dBWinH >> 3);
        hipLaunchKernelGGL(yk_dec_zero_unmarked_batch_win_kernel, dim3((nWin + 255) / 256, 3, (unsigned)c->dFrames), dim3(256), 0, c->stream, c->dB.tile4, c->dStride.tile4,
                           c->dTile4Size, (w + 15) >> 4, w >> 3, reinterpret_cast<const DWinRect*>(c->dBWinTab.p), wtW, nWin, c->dB.planes, c->dStride.planes, c->dPlaneSize);
    } else if (c->dWinSet) {                                                    // a window is a single image's
        const uint32_t wtW = (uint32_t)(c->dWinW >> 3), nWin = wtW * (uint32_t)(c->dWinH >> 3);
        hipLaunchKernelGGL(yk_dec_zero_unmarked_win_kernel, dim3((nWin + 255) / 256, 3), dim3(256), 0, c->stream, c->dB.tile4, c->dTile4Size, c->dSplit ? 1 : 0,
                           (w + 15) >> 4, w >> 3, (uint32_t)(c->dWinX >> 3), (uint32_t)(c->dWinY >> 3), wtW, nWin, c->dB.planes, c->dPlaneSize);
    } else if (c->dFrames == 1)
        hipLaunchKernelGGL(yk_dec_zero_unmarked_kernel, dim3((unsigned)((T8 + 255) / 256), 3), dim3(256), 0, c->stream, c->dB.tile4, c->dTile4Size, c->dSplit ? 1 : 0,
                           (w + 15) >> 4, w >> 3, T8, c->dB.planes, c->dPlaneSize);
    else                                                                        // the flag is the handle's: what it says holds for every frame
        hipLaunchKernelGGL(yk_dec_zero_unmarked_batch_kernel, dim3((unsigned)((T8 + 255) / 256), 3, (unsigned)c->dFrames), dim3(256), 0, c->stream, c->dB.tile4, c->dStride.tile4,
                           c->dTile4Size, (w + 15) >> 4, w >> 3, T8, c->dB.planes, c->dStride.planes, c->dPlaneSize);
    YK_HIP(c, hipGetLastError());
    c->dPlanesStale = false;
    return YK_OK;
}


static void yk_dec_free_frames(yk_ctx* c) {
    c->dFrm = yk_ctx::DFrames(); c->dB = {};
    c->dw = c->dh = 0; c->dFrames = 1; c->dCur = 0;
    c->dPrepared = false;                                                       // a prepared image lives in these buffers: it goes with them
}

}  // extern "C"
// What yk_decode_prepare_device leaves for yk_decode_render_windows_device (valid while c->dPrepared): the plan of the gradient passes with its
// bitmaps pointing at the handle's copies, the copies of the 1-D streams, the per-tile and per-block offsets of the 1-D count and scan, and one
// bit per 64x64 block that has been rendered.  mapRGB and tile4x4Mask are the image's own arrays.  The buffers are grow-only.
struct YkDecPrepared {
    DecPlan pl = {};
    YkBuf<uint8_t> streams;                                  // [bitmap of pass 0] .. [bitmap of pass n-1][type][pix], each on a multiple of 16
    YkBuf<uint32_t> d1;                                      // [blockTiles][blockPix][totals][offInBlk]
    YkBuf<uint32_t> table;                                   // a render call's [block list][window origins]
    bool has1d = false;
    const uint8_t* type = nullptr; const uint8_t* pix = nullptr; size_t typeBytes = 0, pixBytes = 0; int invRange = 0;
    uint32_t* bT = nullptr; uint32_t* bP = nullptr; uint32_t* tot = nullptr; uint32_t* offInBlk = nullptr;
    YkWindowBlocks blocks;
    std::vector<uint32_t> list;
};
void yk_dec_prepared_free(yk_ctx* c) { delete c->dPrep; c->dPrep = nullptr; c->dPrepared = false; }
void yk_dec_ring_free(yk_ctx* c) {
    for (int i = 0; i < 4; i++) {
        if (c->dTabHost[i]) { (void)hipHostFree(c->dTabHost[i]); c->dTabHost[i] = nullptr; c->dTabHostBytes[i] = 0; }
        if (c->dTabEv[i]) { (void)hipEventDestroy(c->dTabEv[i]); c->dTabEv[i] = nullptr; }
    }
}
extern "C" {

// Every per-image array nFrames times back to back, frame f at base + f * stride; strides are multiples of 16 bytes (the lattice is read a word
// at a time, tile4x4Mask is marked with 32-bit atomics).  Buffers are kept while the shape and the frame count stay the same: only the clears run.
static int yk_dec_begin(yk_ctx* c, int w, int h, int nFrames) {
    // the sizes the encoder accepts (yk_set_image).  At sides of 8 (mod 16) the 8x8-tiled planes have an odd tileW = w >> 3, the tile4x4Mask stride
    // stays (w + 15) >> 4 (its last byte of a row holds one 8x8 tile) and every tile that reaches past the right or bottom edge is skipped
    if (w < 8 || h < 8 || (w & 7) || (h & 7) || w > 32760 || h > 32760) return yk_fail(c, YK_ERR_BAD_ARG, "decode needs width/height multiples of 8 in 8..32760");
    YK_HIP(c, hipSetDevice(c->device));
    const size_t lat = (size_t)(w / 4 + 1) * (h / 4 + 1), N = (size_t)nFrames;
    auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    if (!yk_dec_begun(c) || c->dw != w || c->dh != h || c->dFrames != nFrames) {   // a stream of images (or batches) of one shape keeps its buffers: only the clears below
        YK_HIP(c, hipStreamSynchronize(c->stream));
        yk_dec_free_frames(c);
        const int tileW = w >> 3, tileH = h >> 3;
        c->dPlaneSize = (size_t)tileW * tileH * 64;
        const int stride4 = (w + 15) >> 4;
        c->dTile4Size = (size_t)((stride4 << 2) * (((h + 7) >> 3) << 1)) >> 3;
        c->dStride.planes = c->dPlaneSize * 3;
        c->dStride.mapRGB = up16(lat * 3 + 4);                                       // + 4: the render reads a corner's three bytes as one word
        c->dStride.owner = up16(lat * 4);
        c->dStride.loaded = up16(lat);
        c->dStride.tile4 = up16(((3 * c->dTile4Size + 3) & ~(size_t)3) + 4);         // three planes once the masks are split
        auto& D = c->dFrm;
        hipError_t e = D.planes.alloc(c->stream, c->dStride.planes * N);
        if (e == hipSuccess) e = D.mapRGB.alloc(c->stream, c->dStride.mapRGB * N);
        if (e == hipSuccess) e = D.owner.alloc(c->stream, c->dStride.owner * N / 4);            // the strides are bytes, multiples of 16
        if (e == hipSuccess) e = D.loaded.alloc(c->stream, c->dStride.loaded * N);
        if (e == hipSuccess) e = D.tile4.alloc(c->stream, c->dStride.tile4 * N);
        if (e != hipSuccess) {                                                       // what was allocated is released: the next begin starts afresh
            (void)hipGetLastError();
            yk_dec_free_frames(c);
            return yk_refuse(c, YK_ERR_HIP, "the decode buffers of this shape and frame count do not fit in device memory");
        }
        c->dB = { D.planes, D.mapRGB, D.owner, D.loaded, D.tile4 };
        c->dw = w; c->dh = h; c->dFrames = nFrames;
    }
    c->dCur = 0;
    c->dWinSet = false; c->dWinX = c->dWinY = c->dWinW = c->dWinH = 0; c->dChunkSeen = false; c->dBatchBegun = false;
    c->dPxSet = false; c->dPxX = c->dPxY = c->dPxW = c->dPxH = 0;
    c->dBWinSet = false; c->dBWinW = c->dBWinH = 0;                             // the table stays queued kernels' to read: the next set writes it behind them
    c->dBRectSet = false; c->dBRectMaxTiles = 0;
    c->dPrepared = false;                                                       // a prepared image ends here; what it kept is overwritten by the next prepare
    // The planes (3 B per pixel: 201 MB at 8192 x 8192, 40 us of every frame) are NOT cleared: every renderer marks what it writes in tile4x4Mask and
    // the 1-D decode writes every unmarked quadrant, so after a whole file nothing stale is left; a flow that stops earlier (or writes without
    // marking: the plane-subset loops) gets the unmarked cells zeroed when it needs them (yk_dec_settle).
    c->dPlanesStale = true;
    YK_HIP(c, hipMemsetAsync(c->dB.mapRGB, 0, c->dStride.mapRGB * N, c->stream));
    YK_HIP(c, hipMemsetAsync(c->dB.loaded, 0, c->dStride.loaded * N, c->stream));
    YK_HIP(c, hipMemsetAsync(c->dB.tile4, 0, c->dStride.tile4 * N, c->stream));
    c->dSplit = false;
    c->dAlphaValid = false; c->dAlphaBatch = false;                             // an 'ALPM' plane belongs to one image (or one batch)
    return YK_OK;
}

int yk_decode_begin(yk_ctx* c, int w, int h) {
    if (!c) return YK_ERR_BAD_ARG;
    return yk_dec_begin(c, w, h, 1);
}

int yk_decode_begin_batch(yk_ctx* c, int w, int h, int nFrames) {
    if (!c) return YK_ERR_BAD_ARG;
    if (nFrames < 1 || nFrames > 1024) return yk_refuse(c, YK_ERR_BAD_ARG, "nFrames must be 1..1024");
    const int rc = yk_dec_begin(c, w, h, nFrames);
    if (rc == YK_OK) c->dBatchBegun = true;
    return rc;
}

// The window of the image begun by yk_decode_begin: from here on the decode calls owe the planes only the pixels inside it (include/yaik_hip.h)
int yk_decode_set_window(yk_ctx* c, int x0, int y0, int ww, int wh) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_window: yk_decode_begin first");
    YK_DEC_NO_PREPARED(c, "yk_decode_set_window");
    if (c->dBatchBegun || c->dFrames > 1) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_window: a window belongs to a single image (yk_decode_begin), not to a batch");
    if (c->dChunkSeen) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_window: a chunk of this image has been decoded already; set the window right after yk_decode_begin");
    if (ww == 0 && wh == 0) { c->dWinSet = false; c->dPxSet = false; c->dWinX = c->dWinY = c->dWinW = c->dWinH = 0; return YK_OK; }
    if (((x0 | y0 | ww | wh) & 7) || x0 < 0 || y0 < 0 || ww < 8 || wh < 8 || x0 > c->dw - ww || y0 > c->dh - wh)
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_set_window: x0, y0, ww, wh must be multiples of 8 with ww, wh >= 8 and the window inside the image");
    c->dWinX = x0; c->dWinY = y0; c->dWinW = ww; c->dWinH = wh; c->dWinSet = true; c->dPxSet = false;
    return YK_OK;
}
// yk_decode_set_window for a rectangle at any pixel offset and size (include/yaik_hip.h): the handle's window becomes the rectangle's
// 8-aligned cover, so every chunk call runs as under yk_decode_set_window(cover); the pixel rectangle is kept for yk_decode_output_window_device
int yk_decode_set_window_px(yk_ctx* c, int x0, int y0, int ww, int wh) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_window_px: yk_decode_begin first");
    YK_DEC_NO_PREPARED(c, "yk_decode_set_window_px");
    if (c->dBatchBegun || c->dFrames > 1) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_window_px: a window belongs to a single image (yk_decode_begin), not to a batch");
    if (c->dChunkSeen) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_window_px: a chunk of this image has been decoded already; set the window right after yk_decode_begin");
    if (ww == 0 && wh == 0) { c->dWinSet = false; c->dPxSet = false; c->dWinX = c->dWinY = c->dWinW = c->dWinH = 0; return YK_OK; }
    if (!yk_wpx_window_ok(x0, y0, ww, wh, c->dw, c->dh))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_set_window_px: x0, y0 >= 0, ww, wh >= 1 and the window inside the image");
    const YkPxCover cx = yk_wpx_cover(x0, ww), cy = yk_wpx_cover(y0, wh);
    c->dWinX = cx.c0; c->dWinY = cy.c0; c->dWinW = cx.cw; c->dWinH = cy.cw; c->dWinSet = true;
    c->dPxX = x0; c->dPxY = y0; c->dPxW = ww; c->dPxH = wh; c->dPxSet = true;
    return YK_OK;
}
// the window rounded out to 64-pixel blocks, clipped to the image: what the gradient render fills
static DWinRect yk_dec_win_rect(const yk_ctx* c) {
    DWinRect r = { c->dWinX & ~63, c->dWinY & ~63, (c->dWinX + c->dWinW + 63) & ~63, (c->dWinY + c->dWinH + 63) & ~63 };
    if (r.x1 > c->dw) r.x1 = c->dw;
    if (r.y1 > c->dh) r.y1 = c->dh;
    return r;
}

int yk_decode_select_frame(yk_ctx* c, int frame) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_begin first");
    if (frame < 0 || frame >= c->dFrames) return yk_refuse(c, YK_ERR_BAD_ARG, "frame out of range");
    c->dCur = frame;
    return YK_OK;
}

// The per-frame tables of a batch call travel through a ring of four pinned host buffers: the call fills one, queues its copy into HBM and records
// an event behind the copy.  A slot is waited for only when it comes round again, i.e. when the tables of four earlier batch calls are still queued.
int yk_dec_table_host(yk_ctx* c, size_t bytes, int* slot, void** host) {
    const int k = (int)(c->dTabSeq++ & 3u);
    if (c->dTabEv[k]) YK_HIP(c, hipEventSynchronize(c->dTabEv[k]));
    else YK_HIP(c, hipEventCreateWithFlags(&c->dTabEv[k], hipEventDisableTiming));
    if (c->dTabHostBytes[k] < bytes) {
        if (c->dTabHost[k]) { (void)hipHostFree(c->dTabHost[k]); c->dTabHost[k] = nullptr; c->dTabHostBytes[k] = 0; }
        YK_HIP(c, hipHostMalloc(&c->dTabHost[k], bytes, hipHostMallocDefault));
        c->dTabHostBytes[k] = bytes;
    }
    *slot = k; *host = c->dTabHost[k];
    return YK_OK;
}
int yk_dec_table_upload(yk_ctx* c, int slot, void* dev, size_t bytes) {
    YK_HIP(c, hipMemcpyAsync(dev, c->dTabHost[slot], bytes, hipMemcpyHostToDevice, c->stream));
    YK_HIP(c, hipEventRecord(c->dTabEv[slot], c->stream));
    return YK_OK;
}

// One window per frame of the batch begun by yk_decode_begin_batch (include/yaik_hip.h).  The rectangles go through the pinned ring
// into a table of the handle's own (not the scratch buffer, which every chunk call lays out anew): the copy is queued on the handle's stream, so the
// kernels of an earlier batch that are still queued read the earlier rectangles, and the ring slot is reused only once its copy has run.
int yk_decode_set_batch_windows(yk_ctx* c, const int* xy, int ww, int wh) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c) || !c->dBatchBegun) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_batch_windows: yk_decode_begin_batch first (the window of a single image is yk_decode_set_window's)");
    if (c->dChunkSeen) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_batch_windows: a chunk of this batch has been decoded already; set the windows right after yk_decode_begin_batch");
    c->dBWinSet = false; c->dBWinW = c->dBWinH = 0; c->dPxSet = false;           // a refusal below leaves the batch without windows
    c->dBRectSet = false; c->dBRectMaxTiles = 0;                                // windows replace rectangles (yk_decode_set_batch_rects)
    if (ww == 0 && wh == 0) return YK_OK;
    if (!xy) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_set_batch_windows: the origin table is NULL");
    const int N = c->dFrames;
    bool ok = !((ww | wh) & 7) && ww >= 8 && wh >= 8 && ww <= c->dw && wh <= c->dh;
    for (int f = 0; ok && f < N; f++) {
        const int x0 = xy[2 * f], y0 = xy[2 * f + 1];
        ok = !((x0 | y0) & 7) && x0 >= 0 && y0 >= 0 && x0 <= c->dw - ww && y0 <= c->dh - wh;
    }
    if (!ok) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_set_batch_windows: x0, y0, ww, wh must be multiples of 8 with ww, wh >= 8 and every frame's window inside the image");
    YK_HIP(c, hipSetDevice(c->device));
    YK_HIP(c, c->dBWinTab.reserve(c->stream, (size_t)1024 * 6));                // every batch fits (yk_decode_set_batch_windows_px adds two ints per frame): allocated once, so no later call waits for queued readers
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, (size_t)N * sizeof(DWinRect), &slot, &host); if (rc) return rc; }
    DWinRect* tab = static_cast<DWinRect*>(host);
    for (int f = 0; f < N; f++) tab[f] = DWinRect{ xy[2 * f], xy[2 * f + 1], xy[2 * f] + ww, xy[2 * f + 1] + wh };
    { const int rc = yk_dec_table_upload(c, slot, c->dBWinTab.p, (size_t)N * sizeof(DWinRect)); if (rc) return rc; }
    c->dBWinW = ww; c->dBWinH = wh; c->dBWinSet = true;
    return YK_OK;
}
// yk_decode_set_batch_windows for rectangles at any pixel offset (include/yaik_hip.h).  The batch kernels take one tile count for every
// frame, so every frame gets the shared cover of yk_window_px.h: the table's rectangles are the covers, which is all the upstream kernels read, and
// the windows' offsets inside their covers follow them in the same upload, for the clipping de-tile alone.
int yk_decode_set_batch_windows_px(yk_ctx* c, const int* xy, int ww, int wh) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c) || !c->dBatchBegun) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_batch_windows_px: yk_decode_begin_batch first (the window of a single image is yk_decode_set_window_px's)");
    if (c->dChunkSeen) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_batch_windows_px: a chunk of this batch has been decoded already; set the windows right after yk_decode_begin_batch");
    c->dBWinSet = false; c->dBWinW = c->dBWinH = 0; c->dPxSet = false;           // a refusal below leaves the batch without windows
    c->dBRectSet = false; c->dBRectMaxTiles = 0;                                // windows replace rectangles (yk_decode_set_batch_rects)
    if (ww == 0 && wh == 0) return YK_OK;
    if (!xy) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_set_batch_windows_px: the origin table is NULL");
    const int N = c->dFrames, w = c->dw, h = c->dh;
    if (!yk_wpx_windows_ok(N, xy, ww, wh, w, h))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_set_batch_windows_px: x0, y0 >= 0, ww, wh >= 1 and every frame's window inside the image");
    bool aligned = true;
    for (int f = 0; aligned && f < N; f++) aligned = yk_wpx_aligned(xy[2 * f], xy[2 * f + 1], ww, wh);
    if (aligned) return yk_decode_set_batch_windows(c, xy, ww, wh);             // every window is its own cover: the aligned kernels
    YK_HIP(c, hipSetDevice(c->device));
    YK_HIP(c, c->dBWinTab.reserve(c->stream, (size_t)1024 * 6));                // the rectangles and the offsets of every batch: allocated once per handle
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, (size_t)N * 6 * sizeof(int), &slot, &host); if (rc) return rc; }
    DWinRect* tab = static_cast<DWinRect*>(host);
    int* off = static_cast<int*>(host) + 4 * (size_t)N;
    for (int f = 0; f < N; f++) {
        const YkPxCover cx = yk_wpx_shared_cover(xy[2 * f], ww, w), cy = yk_wpx_shared_cover(xy[2 * f + 1], wh, h);
        tab[f] = DWinRect{ cx.c0, cy.c0, cx.c0 + cx.cw, cy.c0 + cy.cw };
        off[2 * f] = xy[2 * f] - cx.c0; off[2 * f + 1] = xy[2 * f + 1] - cy.c0;
    }
    { const int rc = yk_dec_table_upload(c, slot, c->dBWinTab.p, (size_t)N * 6 * sizeof(int)); if (rc) return rc; }
    c->dBWinW = yk_wpx_shared_size(ww, w); c->dBWinH = yk_wpx_shared_size(wh, h); c->dBWinSet = true;
    c->dPxW = ww; c->dPxH = wh; c->dPxSet = true;
    return YK_OK;
}
static const DWinRect* yk_dec_bwin_tab(const yk_ctx* c) { return reinterpret_cast<const DWinRect*>(c->dBWinTab.p); }

// One source rectangle per frame, each of its own size (include/yaik_hip.h).  The taps of a resampled output never leave the rectangle,
// so frame f's window for the chunk calls is the rectangle's own 8-aligned cover: the covers go where windows go (dBWinTab, through the pinned ring)
// and the kernels that took one tile count for the batch have siblings that read frame f's own.  The exact rectangles stay on the host.
int yk_decode_set_batch_rects(yk_ctx* c, const int* rects) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c) || !c->dBatchBegun) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_batch_rects: yk_decode_begin_batch first (a single image takes its rectangle in yk_decode_output_resampled_device)");
    if (c->dChunkSeen) return yk_refuse(c, YK_ERR_STATE, "yk_decode_set_batch_rects: a chunk of this batch has been decoded already; set the rectangles right after yk_decode_begin_batch");
    c->dBWinSet = false; c->dBWinW = c->dBWinH = 0; c->dPxSet = false;           // rectangles replace windows; a refusal below leaves the batch with neither
    c->dBRectSet = false; c->dBRectMaxTiles = 0;
    if (!rects) return YK_OK;
    const int N = c->dFrames, w = c->dw, h = c->dh;
    for (int f = 0; f < N; f++)
        if (!yk_rs_src_ok(rects[4 * f], rects[4 * f + 1], rects[4 * f + 2], rects[4 * f + 3], w, h))
            return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_set_batch_rects: x0, y0 >= 0, 1 <= sw, sh <= 16384 and every frame's rectangle inside the image");
    YK_HIP(c, hipSetDevice(c->device));
    YK_HIP(c, c->dBWinTab.reserve(c->stream, (size_t)1024 * 6));                // the table of the window calls: allocated once per handle
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, (size_t)N * sizeof(DWinRect), &slot, &host); if (rc) return rc; }
    DWinRect* tab = static_cast<DWinRect*>(host);
    int mw = 0, mh = 0; uint32_t mt = 0;
    for (int f = 0; f < N; f++) {
        const YkRsCover k = yk_rs_cover(rects[4 * f], rects[4 * f + 1], rects[4 * f + 2], rects[4 * f + 3]);
        tab[f] = DWinRect{ k.x0, k.y0, k.x1, k.y1 };
        const int cw = k.x1 - k.x0, ch = k.y1 - k.y0;
        const uint32_t t = (uint32_t)(cw >> 3) * (uint32_t)(ch >> 3);
        mw = cw > mw ? cw : mw; mh = ch > mh ? ch : mh; mt = t > mt ? t : mt;
    }
    { const int rc = yk_dec_table_upload(c, slot, c->dBWinTab.p, (size_t)N * sizeof(DWinRect)); if (rc) return rc; }
    c->dBRects.assign(rects, rects + 4 * (size_t)N);
    c->dBWinW = mw; c->dBWinH = mh; c->dBWinSet = true;
    c->dBRectMaxTiles = mt; c->dBRectSet = true;
    return YK_OK;
}

// PaletteFullRangeRemapping (decoder/YAIK_GenericFunctions.cpp:128-137) of a corner stream that is still in HBM: v * ((255 << 16) / range) >> 16
static uint32_t yk_dec_remap_factor(int remapRange) { return remapRange > 0 ? (uint32_t)((255u << 16) / (uint32_t)remapRange) : 0u; }
__global__ void yk_dec_remap_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t n, uint32_t factor) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = (uint8_t)(((uint32_t)src[i] * factor) >> 16);
}

// ---- what the gradient entry points share; the checks and their messages stay with the callers ---------------------------------------------
// length in bytes of the tile bitmap of a (sx, sy) pass over a w x h image; 0: not one of the seven tile formats 16x16 .. 4x4 (sides 1:1, 2:1 or 1:2)
static size_t yk_dpass_bytes(int sx, int sy, int w, int h) {
    if (sx < 2 || sx > 4 || sy < 2 || sy > 4 || sx - sy > 1 || sy - sx > 1) return 0;
    const DPassGeo g = yk_dpass_geo(sx, sy, w);
    return ((size_t)g.xBB * ((h + g.bigY - 1) / g.bigY) * g.bitCount) >> 3;
}
// the first-toucher key of the all-passes kernels is pass << 27 | tile slot << 2 | corner: a pass has to stay below 2^25 tile slots
static bool yk_dpass_fits_key(size_t need) { return need * 8 < ((size_t)1 << 25); }
// the part of a (zeroed) DecPlan that the shape of the image and the order of the passes decide; passes past nPasses are empty 16x16 ones
static void yk_dplan_shape(DecPlan& pl, int nPasses, const int* sx, const int* sy, const size_t* need) {
    pl.n = nPasses;
    for (int p = 0; p < 7; p++) {
        const size_t nb = p < nPasses ? need[p] : 0;
        pl.nBytes[p] = (uint32_t)nb;
        pl.sx[p] = p < nPasses ? sx[p] : 4; pl.sy[p] = p < nPasses ? sy[p] : 4;
        pl.byteStart[p + 1] = pl.byteStart[p] + (uint32_t)nb;
        pl.blockStart[p + 1] = pl.blockStart[p] + (uint32_t)((nb + 1023) / 1024);
    }
}
// scratch of one frame of an all-passes call: [corners per 1024-byte block | ownership bits per bitmap byte (one word)], a multiple of 16 bytes
struct DecAllScratch { size_t oSums, oPerThread, bytes; };
static DecAllScratch yk_decall_scratch(const DecPlan& pl) {
    const size_t oPerThread = (size_t)pl.blockStart[7] * 4;
    return { 0, oPerThread, (oPerThread + (size_t)pl.byteStart[7] * 4 + 15) & ~(size_t)15 };
}
// the inputs of the per-pass kernels in scratch, [bitmap, padded to whole words][colours][corners per block of 1024 tile slots][total]: the bitmap
// behind a clear of its last word, the colours copied or (remapRange > 0, a stream in HBM) remapped on the way; the owner lattice is cleared
struct DPassIn { size_t nWords, nBits, nb; const uint32_t* bm; const uint8_t* rgb; uint32_t* blockSums; uint32_t* total; };
static hipError_t yk_dpass_stage(yk_ctx* c, const uint8_t* bitmap, size_t need, const uint8_t* rgb, size_t rgbBytes, hipMemcpyKind kind, int remapRange, DPassIn* in) {
    const size_t nWords = (need + 3) / 4, nBits = need * 8, nb = (nBits + 1023) / 1024;
    const size_t oB = 0, oR = oB + nWords * 4 + 16, oBB = (oR + rgbBytes + 19) & ~(size_t)15, oT = oBB + nb * 4 + 16;
    hipError_t e = c->dScratch.reserve(c->stream, oT + 64);
    uint8_t* S = c->dScratch;
    if (e == hipSuccess) e = hipMemsetAsync(S + oB, 0, nWords * 4, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(S + oB, bitmap, need, kind, c->stream);
    if (e == hipSuccess && rgbBytes) {
        if (remapRange > 0)
            hipLaunchKernelGGL(yk_dec_remap_kernel, dim3((unsigned)((rgbBytes + 255) / 256 < 1024 ? (rgbBytes + 255) / 256 : 1024)), dim3(256), 0, c->stream,
                               rgb, S + oR, rgbBytes, yk_dec_remap_factor(remapRange));
        else e = hipMemcpyAsync(S + oR, rgb, rgbBytes, kind, c->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(yk_dec_frame(c).owner, 0xFF, (size_t)(c->dw / 4 + 1) * (c->dh / 4 + 1) * 4, c->stream);
    *in = { nWords, nBits, nb, reinterpret_cast<const uint32_t*>(S + oB), S + oR, reinterpret_cast<uint32_t*>(S + oBB), reinterpret_cast<uint32_t*>(S + oT) };
    return e;
}

static int yk_decode_gradient_impl(yk_ctx* c, int sx, int sy, const uint8_t* bitmap, size_t bitmapBytes, const uint8_t* rgb, size_t rgbBytes, bool onDevice, int remapRange) {
    if (!c || !bitmap) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    YK_DEC_NO_PREPARED(c, "yk_decode_gradient[_device]");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_gradient[_device]");
    const YkDecView V = yk_dec_frame(c);
    const int w = c->dw, h = c->dh, latW = w / 4 + 1;
    const size_t need = yk_dpass_bytes(sx, sy, w, h);
    if (!need) return yk_fail(c, YK_ERR_BAD_ARG, "unsupported tile format");
    YK_HIP(c, hipSetDevice(c->device));
    if (bitmapBytes < need) return yk_fail(c, YK_ERR_RANGE, "tile bitmap shorter than the image needs");
    c->dChunkSeen = true;
    const DPassGeo g = yk_dpass_geo(sx, sy, w);
    DPassIn in;
    YK_HIP(c, yk_dpass_stage(c, bitmap, need, rgb, rgbBytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, onDevice ? remapRange : 0, &in));
    { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
    hipLaunchKernelGGL(yk_dec_owner_kernel, dim3((unsigned)((in.nBits + 255) / 256)), dim3(256), 0, c->stream, in.bm, in.nBits, g, w, h, latW, V.loaded, V.owner);
    hipLaunchKernelGGL(yk_dec_corner_kernel<false>, dim3((unsigned)in.nb), dim3(1024), 0, c->stream, in.bm, in.nBits, g, w, h, latW, V.loaded, V.owner,
                       in.blockSums, (const uint8_t*)nullptr, (size_t)0, (uint8_t*)nullptr);
    hipLaunchKernelGGL(yk_u32_scanblocks_kernel, dim3(1), dim3(1024), 0, c->stream, in.blockSums, (int)in.nb, in.total);
    hipLaunchKernelGGL(yk_dec_corner_kernel<true>, dim3((unsigned)in.nb), dim3(1024), 0, c->stream, in.bm, in.nBits, g, w, h, latW, V.loaded, V.owner,
                       in.blockSums, in.rgb, rgbBytes, V.mapRGB);
    if (c->dWinSet)
        hipLaunchKernelGGL(yk_dec_render_win_kernel, dim3((unsigned)in.nWords), dim3(256), 0, c->stream, in.bm, in.nWords, g, w, h, latW, V.mapRGB, V.planes, c->dPlaneSize,
                           w >> 3, reinterpret_cast<uint32_t*>(V.tile4), (w + 15) >> 4, yk_dec_win_rect(c));
    else
        hipLaunchKernelGGL(yk_dec_render_kernel, dim3((unsigned)in.nWords), dim3(256), 0, c->stream, in.bm, in.nWords, g, w, h, latW, V.mapRGB, V.planes, c->dPlaneSize,
                           w >> 3, reinterpret_cast<uint32_t*>(V.tile4), (w + 15) >> 4);
    YK_HIP(c, hipGetLastError());
    { int rc2 = yk_stage_end(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
    if (!onDevice) YK_HIP(c, hipStreamSynchronize(c->stream));            // the host buffers may be reused by the caller
    return YK_OK;
}

int yk_decode_gradient(yk_ctx* c, int sx, int sy, const uint8_t* bitmap, size_t bitmapBytes, const uint8_t* rgb, size_t rgbBytes) {
    return yk_decode_gradient_impl(c, sx, sy, bitmap, bitmapBytes, rgb, rgbBytes, false, 0);
}

int yk_decode_gradient_device(yk_ctx* c, int sx, int sy, const uint8_t* devBitmap, size_t bitmapBytes, const uint8_t* devRgb, size_t rgbBytes, int remapRange) {
    return yk_decode_gradient_impl(c, sx, sy, devBitmap, bitmapBytes, devRgb, rgbBytes, true, remapRange);
}

int yk_decode_gradient_all_device(yk_ctx* c, int nPasses, const int* tileShiftX, const int* tileShiftY, const uint8_t* const* devBitmap, const size_t* bitmapBytes,
                                  const uint8_t* const* devRgb, const size_t* rgbBytes, int remapRange) {
    if (!c || nPasses < 0 || (nPasses && (!tileShiftX || !tileShiftY || !devBitmap || !bitmapBytes || !devRgb || !rgbBytes))) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    YK_DEC_NO_PREPARED(c, "yk_decode_gradient_all_device");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_gradient_all_device");
    const YkDecView V = yk_dec_frame(c);
    if (nPasses == 0) return YK_OK;
    const int w = c->dw, h = c->dh, latW = w / 4 + 1;
    const size_t lat = (size_t)latW * (h / 4 + 1);
    bool oneCall = nPasses <= 7;
    size_t need[7] = {};
    for (int p = 0; p < nPasses; p++) {
        const size_t n = yk_dpass_bytes(tileShiftX[p], tileShiftY[p], w, h);
        if (!n) return yk_fail(c, YK_ERR_BAD_ARG, "unsupported tile format");
        if (!devBitmap[p] || (rgbBytes[p] && !devRgb[p])) return yk_fail(c, YK_ERR_BAD_ARG, "NULL tile bitmap, or NULL colour stream with a length");
        if (p < 7) {                                                         // a later chunk is checked by its own pass-after-pass call
            need[p] = n;
            if (bitmapBytes[p] < n) return yk_fail(c, YK_ERR_RANGE, "tile bitmap shorter than the image needs");
            if (!yk_dpass_fits_key(n) || rgbBytes[p] > 0xFFFFFFFFu) oneCall = false;
        }
    }
    if (!oneCall) {                                                          // very large images / more than seven chunks: pass after pass
        for (int p = 0; p < nPasses; p++) {
            const int rc = yk_decode_gradient_impl(c, tileShiftX[p], tileShiftY[p], devBitmap[p], bitmapBytes[p], devRgb[p], rgbBytes[p], true, remapRange);
            if (rc) return rc;
        }
        return YK_OK;
    }
    YK_HIP(c, hipSetDevice(c->device));
    c->dChunkSeen = true;
    DecPlan pl = {};
    yk_dplan_shape(pl, nPasses, tileShiftX, tileShiftY, need);
    for (int p = 0; p < nPasses; p++) { pl.bm[p] = devBitmap[p]; pl.rgb[p] = devRgb[p]; pl.rgbBytes[p] = (uint32_t)rgbBytes[p]; }
    const size_t nbTot = pl.blockStart[7], nBytesTot = pl.byteStart[7];
    const DecAllScratch L = yk_decall_scratch(pl);
    { const int rc = yk_dec_scratch(c, L.bytes); if (rc) return rc; }
    uint32_t* blockSums = reinterpret_cast<uint32_t*>(c->dScratch + L.oSums);
    uint32_t* perThread = reinterpret_cast<uint32_t*>(c->dScratch + L.oPerThread);
    YK_HIP(c, hipMemsetAsync(V.owner, 0xFF, lat * 4, c->stream));
    { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
    // 1 clear + 5 launches for all passes (the per-pass form: 3 copies / clears + 5 launches per pass)
    hipLaunchKernelGGL(yk_decall_owner_kernel, dim3((unsigned)((nBytesTot + 255) / 256)), dim3(256), 0, c->stream, pl, w, h, latW, V.loaded, V.owner);
    hipLaunchKernelGGL(yk_decall_stream_kernel<false>, dim3((unsigned)nbTot), dim3(1024), 0, c->stream, pl, w, h, latW, V.loaded, V.owner, blockSums, perThread,
                       (uint8_t*)nullptr, 0u);
    hipLaunchKernelGGL(yk_decall_scan_kernel, dim3(1), dim3(1024), 0, c->stream, blockSums, pl);
    hipLaunchKernelGGL(yk_decall_stream_kernel<true>, dim3((unsigned)nbTot), dim3(1024), 0, c->stream, pl, w, h, latW, V.loaded, V.owner, blockSums, perThread,
                       V.mapRGB, yk_dec_remap_factor(remapRange));
    // the render: a workgroup per 64x64 block of the image walks the passes in call order
    if (c->dWinSet)
        hipLaunchKernelGGL(yk_decall_render_blocks_win_kernel, dim3((unsigned)(((w + 63) / 64) * ((h + 63) / 64))), dim3(256), 0, c->stream, pl, w, h, latW,
                           V.mapRGB, V.planes, c->dPlaneSize, w >> 3, reinterpret_cast<uint32_t*>(V.tile4), (w + 15) >> 4, yk_dec_win_rect(c));
    else
        hipLaunchKernelGGL(yk_decall_render_blocks_kernel, dim3((unsigned)(((w + 63) / 64) * ((h + 63) / 64))), dim3(256), 0, c->stream, pl, w, h, latW,
                           V.mapRGB, V.planes, c->dPlaneSize, w >> 3, reinterpret_cast<uint32_t*>(V.tile4), (w + 15) >> 4);
    YK_HIP(c, hipGetLastError());
    { int rc2 = yk_stage_end(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
    return YK_OK;
}

// The same over every frame of the batch begun by yk_decode_begin_batch: one clear, one table copy and the five launches, each over nFrames x blocks.
int yk_decode_gradient_all_batch_device(yk_ctx* c, int nPasses, const int* tileShiftX, const int* tileShiftY, const uint8_t* const* devBitmap, const size_t* bitmapBytes,
                                        const uint8_t* const* devRgb, const size_t* rgbBytes, int remapRange) {
    if (!c) return YK_ERR_BAD_ARG;
    if (nPasses < 0 || nPasses > 7) return yk_refuse(c, YK_ERR_BAD_ARG, "a batch takes 0..7 gradient passes per call");
    if (nPasses && (!tileShiftX || !tileShiftY || !devBitmap || !bitmapBytes || !devRgb || !rgbBytes)) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL table");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_begin_batch first");
    YK_DEC_NO_PREPARED(c, "yk_decode_gradient_all_batch_device");
    if (nPasses == 0) return YK_OK;
    const int w = c->dw, h = c->dh, latW = w / 4 + 1, N = c->dFrames;
    size_t need[7] = {};
    for (int p = 0; p < nPasses; p++) {
        if (!(need[p] = yk_dpass_bytes(tileShiftX[p], tileShiftY[p], w, h))) return yk_refuse(c, YK_ERR_BAD_ARG, "unsupported tile format");
        if (!yk_dpass_fits_key(need[p])) return yk_refuse(c, YK_ERR_BAD_ARG, "a pass of 2^25 tile slots or more does not fit a batch (decode such images one by one)");
        if (bitmapBytes[p] < need[p]) return yk_refuse(c, YK_ERR_RANGE, "tile bitmap shorter than the image needs");
    }
    for (size_t i = 0; i < (size_t)N * nPasses; i++) {
        if (!devBitmap[i]) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL tile bitmap");
        if (rgbBytes[i] && !devRgb[i]) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL colour stream with a length");
        if (rgbBytes[i] > 0xFFFFFFFFu) return yk_refuse(c, YK_ERR_BAD_ARG, "colour stream of 4 GB or more");
    }
    YK_HIP(c, hipSetDevice(c->device));
    if (c->dBatchBegun) c->dChunkSeen = true;                                 // from here on yk_decode_set_batch_windows refuses
    DecPlan pl = {};                                                          // what the frames share: the geometry
    yk_dplan_shape(pl, nPasses, tileShiftX, tileShiftY, need);
    const size_t nbTot = pl.blockStart[7], nBytesTot = pl.byteStart[7];
    // scratch: [plan table] then per frame, at a fixed stride, the arrays of yk_decode_gradient_all_device
    const size_t tabBytes = ((size_t)N * sizeof(DecPlan) + 255) & ~(size_t)255;
    const DecAllScratch L = yk_decall_scratch(pl);
    { const int rc = yk_dec_scratch(c, tabBytes + (size_t)N * L.bytes); if (rc) return rc; }
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, (size_t)N * sizeof(DecPlan), &slot, &host); if (rc) return rc; }
    DecPlan* tab = static_cast<DecPlan*>(host);
    for (int f = 0; f < N; f++) {
        tab[f] = pl;
        for (int p = 0; p < nPasses; p++) {
            const size_t i = (size_t)f * nPasses + p;
            tab[f].bm[p] = devBitmap[i]; tab[f].rgb[p] = devRgb[i]; tab[f].rgbBytes[p] = (uint32_t)rgbBytes[i];
        }
    }
    { const int rc = yk_dec_table_upload(c, slot, c->dScratch, (size_t)N * sizeof(DecPlan)); if (rc) return rc; }
    DecBatch B;
    B.plans = reinterpret_cast<const DecPlan*>(c->dScratch.p);
    B.loaded = c->dB.loaded; B.owner = reinterpret_cast<uint8_t*>(c->dB.owner); B.mapRGB = c->dB.mapRGB; B.planes = c->dB.planes; B.tile4 = c->dB.tile4;
    B.scratch = c->dScratch + tabBytes;
    B.sLoaded = c->dStride.loaded; B.sOwner = c->dStride.owner; B.sMapRGB = c->dStride.mapRGB; B.sPlanes = c->dStride.planes; B.sTile4 = c->dStride.tile4; B.sScratch = L.bytes;
    B.oSums = L.oSums; B.oPerThread = L.oPerThread;
    const unsigned F = (unsigned)N;
    YK_HIP(c, hipMemsetAsync(c->dB.owner, 0xFF, c->dStride.owner * (size_t)N, c->stream));
    { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
    hipLaunchKernelGGL(yk_decall_owner_batch_kernel, dim3((unsigned)((nBytesTot + 255) / 256), F), dim3(256), 0, c->stream, B, w, h, latW);
    hipLaunchKernelGGL(yk_decall_stream_batch_kernel<false>, dim3((unsigned)nbTot, F), dim3(1024), 0, c->stream, B, w, h, latW, 0u);
    hipLaunchKernelGGL(yk_decall_scan_batch_kernel, dim3(F), dim3(1024), 0, c->stream, B);
    hipLaunchKernelGGL(yk_decall_stream_batch_kernel<true>, dim3((unsigned)nbTot, F), dim3(1024), 0, c->stream, B, w, h, latW, yk_dec_remap_factor(remapRange));
    if (c->dBWinSet)                                                          // the map-sized work above stays whole; the blocks outside a frame's window are marked, not rendered
        hipLaunchKernelGGL(yk_decall_render_blocks_batch_win_kernel, dim3((unsigned)(((w + 63) / 64) * ((h + 63) / 64)), F), dim3(256), 0, c->stream, B, yk_dec_bwin_tab(c),
                           w, h, latW, c->dPlaneSize, w >> 3, (w + 15) >> 4);
    else
        hipLaunchKernelGGL(yk_decall_render_blocks_batch_kernel, dim3((unsigned)(((w + 63) / 64) * ((h + 63) / 64)), F), dim3(256), 0, c->stream, B, w, h, latW,
                           c->dPlaneSize, w >> 3, (w + 15) >> 4);
    YK_HIP(c, hipGetLastError());
    { int rc2 = yk_stage_end(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
    return YK_OK;
}

static int yk_dec_split(yk_ctx* c) {                                       // UpdateTileAndRGBMask (YAIK_API.cpp:530-544), once
    if (c->dSplit) return YK_OK;
    const YkDecView V = yk_dec_frame(c);
    const size_t lat = (size_t)(c->dw / 4 + 1) * (c->dh / 4 + 1), n = lat > c->dTile4Size ? lat : c->dTile4Size;
    hipLaunchKernelGGL(yk_dec_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, V.loaded, lat, V.tile4, c->dTile4Size);
    YK_HIP(c, hipGetLastError());
    c->dSplit = true;
    return YK_OK;
}

int yk_decode_split_masks(yk_ctx* c) {
    if (!c) return YK_ERR_BAD_ARG;
    YK_DEC_NO_BATCH(c, "yk_decode_split_masks");
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    YK_DEC_NO_PREPARED(c, "yk_decode_split_masks");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_split_masks");
    YK_HIP(c, hipSetDevice(c->device));
    c->dChunkSeen = true;
    return yk_dec_split(c);
}

int yk_decode_gradient_planes(yk_ctx* c, int planeBit, int consistentMarks, const uint8_t* bitmap, size_t bitmapBytes, const uint8_t* rgb, size_t rgbBytes) {
    if (!c || !bitmap) return YK_ERR_BAD_ARG;
    YK_DEC_NO_BATCH(c, "yk_decode_gradient_planes");
    YK_DEC_NO_PREPARED(c, "yk_decode_gradient_planes");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_gradient_planes");
    if (planeBit == 7) return yk_decode_gradient(c, 2, 2, bitmap, bitmapBytes, rgb, rgbBytes);
    if (planeBit < 1 || planeBit > 6) return yk_fail(c, YK_ERR_BAD_ARG, "planeBit must be 1..7");
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    const YkDecView V = yk_dec_frame(c);
    YK_HIP(c, hipSetDevice(c->device));
    c->dChunkSeen = true;
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }               // the plane-subset loops write without marking (reference behaviour): from here on the planes are fully defined
    const int w = c->dw, h = c->dh, latW = w / 4 + 1;
    const size_t lat = (size_t)latW * (h / 4 + 1);
    const size_t need = yk_dpass_bytes(2, 2, w, h);                          // 4x4 tiles
    if (bitmapBytes < need) return yk_fail(c, YK_ERR_RANGE, "tile bitmap shorter than the image needs");
    { const int rc = yk_dec_split(c); if (rc) return rc; }                   // a chunk whose plane field is not 7 splits the masks first (:875-877)
    DPassIn in;
    YK_HIP(c, yk_dpass_stage(c, bitmap, need, rgb, rgbBytes, hipMemcpyHostToDevice, 0, &in));
    const unsigned g256 = (unsigned)((in.nBits + 255) / 256);
    hipLaunchKernelGGL(yk_dec44p_owner_kernel, dim3(g256), dim3(256), 0, c->stream, in.bm, in.nBits, w, h, latW, planeBit, V.loaded, V.owner);
    hipLaunchKernelGGL(yk_dec44p_corner_kernel<false>, dim3((unsigned)in.nb), dim3(1024), 0, c->stream, in.bm, in.nBits, w, h, latW, planeBit, V.loaded, V.owner,
                       in.blockSums, (const uint8_t*)nullptr, (size_t)0, (uint8_t*)nullptr);
    hipLaunchKernelGGL(yk_u32_scanblocks_kernel, dim3(1), dim3(1024), 0, c->stream, in.blockSums, (int)in.nb, in.total);
    hipLaunchKernelGGL(yk_dec44p_corner_kernel<true>, dim3((unsigned)in.nb), dim3(1024), 0, c->stream, in.bm, in.nBits, w, h, latW, planeBit, V.loaded, V.owner,
                       in.blockSums, in.rgb, rgbBytes, V.mapRGB);
    hipLaunchKernelGGL(yk_dec44p_mark_kernel, dim3((unsigned)((lat + 255) / 256)), dim3(256), 0, c->stream, V.owner, lat, planeBit, V.loaded);
    hipLaunchKernelGGL(yk_dec44p_render_kernel, dim3(g256), dim3(256), 0, c->stream, in.bm, in.nBits, w, h, latW, planeBit, consistentMarks, V.mapRGB, V.planes,
                       c->dPlaneSize, w >> 3, reinterpret_cast<uint32_t*>(V.tile4), c->dTile4Size, (w + 15) >> 4);
    YK_HIP(c, hipGetLastError());
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

__global__ void yk_dec1d_next_plane_kernel(uint32_t* __restrict__ runBase, const uint32_t* __restrict__ tot) { if (threadIdx.x < 2) runBase[threadIdx.x] += tot[threadIdx.x]; }

static int yk_decode_1d_impl(yk_ctx* c, const uint8_t* typeStream, size_t typeBytes, const uint8_t* pixStream, size_t pixBytes, int compressionRange, bool onDevice) {
    if (!c || !typeStream || !pixStream || compressionRange <= 0) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    YK_DEC_NO_PREPARED(c, "yk_decode_1d[_device]");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_1d[_device]");
    const YkDecView V = yk_dec_frame(c);
    YK_HIP(c, hipSetDevice(c->device));
    c->dChunkSeen = true;
    // dPlanesStale is the handle's: this call writes the unmarked quadrants of the SELECTED frame only, so on a batch the other frames get theirs zeroed first
    if (c->dFrames > 1) { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    const int w = c->dw, h = c->dh, tilesW = w >> 3;
    const size_t T8 = (size_t)tilesW * (h >> 3), nb = (T8 + 1023) / 1024;
    const size_t oTy = 0, oPx = (oTy + typeBytes + 31) & ~(size_t)15, oCT = (oPx + pixBytes + 31) & ~(size_t)15, oCP = oCT + 16,
                 oBT = oCP + 16, oBP = oBT + nb * 4 + 16, oTot = oBP + nb * 4 + 16, oOff = oTot + 64;
    int rc = yk_dec_scratch(c, oOff + T8 * 4 + 64); if (rc) return rc;
    uint8_t* S = c->dScratch;
    // streams that already lie in HBM (16-byte aligned, as the encoder leaves them) are read where they are
    const bool inPlace = onDevice && ((reinterpret_cast<uintptr_t>(typeStream) | reinterpret_cast<uintptr_t>(pixStream)) & 15) == 0;
    if (!inPlace) {
        YK_HIP(c, hipMemcpyAsync(S + oTy, typeStream, typeBytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        YK_HIP(c, hipMemcpyAsync(S + oPx, pixStream, pixBytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    }
    const uint8_t* const tyS = inPlace ? typeStream : S + oTy; const uint8_t* const pxS = inPlace ? pixStream : S + oPx;
    uint32_t* bT = reinterpret_cast<uint32_t*>(S + oBT); uint32_t* bP = reinterpret_cast<uint32_t*>(S + oBP);
    uint32_t* tot = reinterpret_cast<uint32_t*>(S + oTot);
    uint32_t* offInBlk = reinterpret_cast<uint32_t*>(S + oOff);
    const unsigned gTiles = (unsigned)((T8 + 64 * YK_D1_TPL - 1) / (64 * YK_D1_TPL));
    { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_1D); if (rc2) return rc2; }
    if (!c->dSplit) {
        // no partial-plane pass ran: the three planes share one mask, one count / scan serves all of them (3 launches)
        hipLaunchKernelGGL(yk_dec1d_count_kernel, dim3((unsigned)nb), dim3(1024), 0, c->stream, V.tile4, (w + 15) >> 4, tilesW, T8, bT, bP, offInBlk);
        hipLaunchKernelGGL(yk_dec1d_scan_kernel, dim3(1), dim3(1024), 0, c->stream, bT, bP, (int)nb, tot);
        if (c->dWinSet) {
            // count and scan stay whole (stream offsets are prefix sums over every tile of the image); only the window's tiles are decoded
            const D1Win wn = { (uint32_t)(c->dWinX >> 3), (uint32_t)(c->dWinY >> 3), (uint32_t)(c->dWinW >> 3), (uint32_t)tilesW };
            const size_t nWin = (size_t)(c->dWinW >> 3) * (c->dWinH >> 3);
            hipLaunchKernelGGL(yk_dec1d_win_kernel, dim3((unsigned)((nWin + 64 * YK_D1_TPL - 1) / (64 * YK_D1_TPL)), 3), dim3(256), 0, c->stream, (const uint32_t*)offInBlk, nWin, wn,
                               bT, bP, tot, tyS, typeBytes, pxS, pixBytes, (1 << 24) / compressionRange, V.planes, c->dPlaneSize);
        } else
            hipLaunchKernelGGL(yk_dec1d_kernel, dim3(gTiles, 3), dim3(256), 0, c->stream, (const uint32_t*)offInBlk, T8, bT, bP, tot,
                               tyS, typeBytes, pxS, pixBytes, (1 << 24) / compressionRange, V.planes, c->dPlaneSize, -1, (const uint32_t*)nullptr);
    } else {
        // per-plane masks (Decompress1D reads tile4x4Mask + planeID * tile4x4MaskSize, YAIK_3DTile.cpp:41): one plane after the other,
        // every plane's streams start where the plane before it stopped
        uint32_t* runBase = tot + 4;
        YK_HIP(c, hipMemsetAsync(runBase, 0, 2 * sizeof(uint32_t), c->stream));
        for (int p = 0; p < 3; p++) {
            const uint8_t* t4 = V.tile4 + (size_t)p * c->dTile4Size;
            hipLaunchKernelGGL(yk_dec1d_count_kernel, dim3((unsigned)nb), dim3(1024), 0, c->stream, t4, (w + 15) >> 4, tilesW, T8, bT, bP, offInBlk);
            hipLaunchKernelGGL(yk_dec1d_scan_kernel, dim3(1), dim3(1024), 0, c->stream, bT, bP, (int)nb, tot);
            hipLaunchKernelGGL(yk_dec1d_kernel, dim3(gTiles, 1), dim3(256), 0, c->stream, (const uint32_t*)offInBlk, T8, bT, bP, tot,
                               tyS, typeBytes, pxS, pixBytes, (1 << 24) / compressionRange, V.planes, c->dPlaneSize, p, (const uint32_t*)runBase);
            hipLaunchKernelGGL(yk_dec1d_next_plane_kernel, dim3(1), dim3(64), 0, c->stream, runBase, (const uint32_t*)tot);
        }
    }
    YK_HIP(c, hipGetLastError());
    { int rc2 = yk_stage_end(c, YK_STAGE_DEC_1D); if (rc2) return rc2; }
    c->dPlanesStale = false;                                                 // every unmarked quadrant of every plane has been written
    if (!onDevice) YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

int yk_decode_1d(yk_ctx* c, const uint8_t* typeStream, size_t typeBytes, const uint8_t* pixStream, size_t pixBytes, int compressionRange) {
    return yk_decode_1d_impl(c, typeStream, typeBytes, pixStream, pixBytes, compressionRange, false);
}

int yk_decode_1d_device(yk_ctx* c, const uint8_t* devType, size_t typeBytes, const uint8_t* devPix, size_t pixBytes, int compressionRange) {
    return yk_decode_1d_impl(c, devType, typeBytes, devPix, pixBytes, compressionRange, true);
}

// The '1DTL' chunk of every frame of a batch: count, scan (one workgroup per frame) and decode, each ONE launch over the frames.  A frame with
// empty streams gets what yk_decode_1d_device gives it when its streams end early: zeros in every quadrant nothing marked, nothing read.
int yk_decode_1d_batch_device(yk_ctx* c, const uint8_t* const* devType, const size_t* typeBytes, const uint8_t* const* devPix, const size_t* pixBytes, int compressionRange) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!devType || !typeBytes || !devPix || !pixBytes) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL table");
    if (compressionRange <= 0) return yk_refuse(c, YK_ERR_BAD_ARG, "compressionRange must be positive");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_begin_batch first");
    YK_DEC_NO_PREPARED(c, "yk_decode_1d_batch_device");
    const int N = c->dFrames;
    for (int f = 0; f < N; f++) {
        if ((typeBytes[f] && !devType[f]) || (pixBytes[f] && !devPix[f])) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL 1-D stream with a length");
        if (pixBytes[f] && (reinterpret_cast<uintptr_t>(devPix[f]) & 15)) return yk_refuse(c, YK_ERR_BAD_ARG, "the pixel streams of a batch are read in place: 16-byte aligned");
    }
    if (c->dSplit) return yk_decode_1d_impl(c, devType[0], typeBytes[0], devPix[0], pixBytes[0], compressionRange, true);   // a batch of one behind a plane-subset chunk: per-plane masks
    YK_HIP(c, hipSetDevice(c->device));
    if (c->dBatchBegun) c->dChunkSeen = true;
    const int w = c->dw, h = c->dh, tilesW = w >> 3;
    const size_t T8 = (size_t)tilesW * (h >> 3), nb = (T8 + 1023) / 1024;
    const size_t tabBytes = ((size_t)N * sizeof(D1Frame) + 255) & ~(size_t)255;
    const size_t oBT = 0, oBP = oBT + nb * 4 + 16, oTot = oBP + nb * 4 + 16, oOff = oTot + 64, sS = (oOff + T8 * 4 + 64 + 15) & ~(size_t)15;
    { const int rc = yk_dec_scratch(c, tabBytes + (size_t)N * sS); if (rc) return rc; }
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, (size_t)N * sizeof(D1Frame), &slot, &host); if (rc) return rc; }
    D1Frame* tab = static_cast<D1Frame*>(host);
    for (int f = 0; f < N; f++) { tab[f].type = devType[f]; tab[f].pix = devPix[f]; tab[f].typeBytes = typeBytes[f]; tab[f].pixBytes = pixBytes[f]; }
    { const int rc = yk_dec_table_upload(c, slot, c->dScratch, (size_t)N * sizeof(D1Frame)); if (rc) return rc; }
    D1Batch B;
    B.frames = reinterpret_cast<const D1Frame*>(c->dScratch.p);
    B.tile4 = c->dB.tile4; B.planes = c->dB.planes; B.scratch = c->dScratch + tabBytes;
    B.sTile4 = c->dStride.tile4; B.sPlanes = c->dStride.planes; B.sScratch = sS;
    B.oBT = oBT; B.oBP = oBP; B.oTot = oTot; B.oOff = oOff;
    const unsigned gTiles = (unsigned)((T8 + 64 * YK_D1_TPL - 1) / (64 * YK_D1_TPL)), F = (unsigned)N;
    { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_1D); if (rc2) return rc2; }
    hipLaunchKernelGGL(yk_dec1d_count_batch_kernel, dim3((unsigned)nb, F), dim3(1024), 0, c->stream, B, (w + 15) >> 4, tilesW, T8);
    hipLaunchKernelGGL(yk_dec1d_scan_batch_kernel, dim3(F), dim3(1024), 0, c->stream, B, (int)nb);
    if (c->dBRectSet)                                                         // ... of its rectangle's own cover: the grid is the largest cover's
        hipLaunchKernelGGL(yk_dec1d_batch_rects_kernel, dim3((c->dBRectMaxTiles + 64 * YK_D1_TPL - 1) / (64 * YK_D1_TPL), 3, F), dim3(256), 0, c->stream, B, yk_dec_bwin_tab(c),
                           (uint32_t)tilesW, (1 << 24) / compressionRange, c->dPlaneSize);
    else if (c->dBWinSet) {                                                   // count and scan stay whole for every frame; only the tiles of its window are decoded
        const uint32_t wtW = (uint32_t)(c->dBWinW >> 3);
        const size_t nWin = (size_t)wtW * (c->dBWinH >> 3);
        hipLaunchKernelGGL(yk_dec1d_batch_win_kernel, dim3((unsigned)((nWin + 64 * YK_D1_TPL - 1) / (64 * YK_D1_TPL)), 3, F), dim3(256), 0, c->stream, B, yk_dec_bwin_tab(c), nWin,
                           wtW, (uint32_t)tilesW, (1 << 24) / compressionRange, c->dPlaneSize);
    } else
        hipLaunchKernelGGL(yk_dec1d_batch_kernel, dim3(gTiles, 3, F), dim3(256), 0, c->stream, B, T8, (1 << 24) / compressionRange, c->dPlaneSize);
    YK_HIP(c, hipGetLastError());
    { int rc2 = yk_stage_end(c, YK_STAGE_DEC_1D); if (rc2) return rc2; }
    c->dPlanesStale = false;                                                 // every unmarked quadrant of every plane of every frame has been written
    return YK_OK;
}

int yk_decode_mask(yk_ctx* c, const uint8_t* bits, int bw, int bh, uint8_t* hostOut, size_t cap) {
    if (!c || !bits || !hostOut || bw <= 0 || bh <= 0) return YK_ERR_BAD_ARG;
    YK_DEC_NO_BATCH(c, "yk_decode_mask");
    const size_t outBytes = (size_t)bw * bh * 32, inBytes = ((size_t)bw * bh + 7) / 8;
    if (cap < outBytes) return yk_fail(c, YK_ERR_RANGE, "mask buffer too small");
    YK_HIP(c, hipSetDevice(c->device));
    const size_t oO = (inBytes + 31) & ~(size_t)15;
    int rc = yk_dec_scratch(c, oO + outBytes + 64); if (rc) return rc;
    YK_HIP(c, hipMemcpyAsync(c->dScratch, bits, inBytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(yk_dec_mask_kernel, dim3((unsigned)((bw * bh + 255) / 256)), dim3(256), 0, c->stream, c->dScratch, bw, bh,
                       reinterpret_cast<unsigned long long*>(c->dScratch + oO));
    YK_HIP(c, hipMemcpyAsync(hostOut, c->dScratch + oO, outBytes, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

int yk_decode_planes(yk_ctx* c, uint8_t* hostR, uint8_t* hostG, uint8_t* hostB, size_t capEach) {
    if (!c || !hostR || !hostG || !hostB) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    const YkDecView V = yk_dec_frame(c);
    if (capEach < c->dPlaneSize) return yk_fail(c, YK_ERR_RANGE, "plane buffer too small");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    uint8_t* dst[3] = { hostR, hostG, hostB };
    for (int p = 0; p < 3; p++) YK_HIP(c, hipMemcpyAsync(dst[p], V.planes + p * c->dPlaneSize, c->dPlaneSize, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

// Shared body of the two output entry points.  The device image is packed tight (w * bpp bytes per row) and lands in the caller's
// buffer by a 2-D copy with dpitch = outputImageStride: like the reference's loop, bytes of a row beyond the pixels are never
// touched (outputImageStride exists to place the image INSIDE a larger buffer, include/YAIK.h:190).
static int yk_decode_output_impl(yk_ctx* c, uint8_t* hostOut, size_t outputImageStride, const uint8_t* hostAlpha, int strideA, bool refRGBA,
                                 const uint8_t* devAlpha = nullptr) {
    if (!c || !hostOut) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    YK_DEC_NO_WINDOW(c, "yk_decode_output / yk_decode_output_alpha / yk_decode_output_reference_rgba");
    if (devAlpha) { hostAlpha = devAlpha; strideA = c->dw; }                   // the plane yk_decode_alpha left in HBM: no host copy
    const int w = c->dw, h = c->dh, bpp = (hostAlpha && !refRGBA) ? 4 : 3;
    const size_t rowBytes = (size_t)w * bpp + (refRGBA && hostAlpha ? 1 : 0);
    if (outputImageStride < rowBytes || (hostAlpha && strideA < w)) return yk_fail(c, YK_ERR_BAD_ARG, "output stride too small");
    YK_HIP(c, hipSetDevice(c->device));
    const size_t dPitch = (rowBytes + 15) & ~(size_t)15;
    const size_t outBytes = dPitch * h, aBytes = (hostAlpha && !devAlpha) ? (size_t)strideA * h : 0, oA = (outBytes + 31) & ~(size_t)15;
    int rc = yk_dec_scratch(c, oA + aBytes + 64); if (rc) return rc;
    rc = yk_dec_settle(c); if (rc) return rc;
    if (hostAlpha && !devAlpha) YK_HIP(c, hipMemcpyAsync(c->dScratch + oA, hostAlpha, aBytes, hipMemcpyHostToDevice, c->stream));
    rc = yk_dec_detile(c, c->dScratch, dPitch, 0, bpp, devAlpha ? devAlpha : bpp == 4 ? c->dScratch + oA : (const uint8_t*)nullptr, (size_t)strideA, 0);
    if (rc) return rc;
    if (refRGBA && hostAlpha) {
        hipLaunchKernelGGL(yk_dec_ref_alpha_kernel, dim3((h + 255) / 256), dim3(256), 0, c->stream, c->dScratch + oA, strideA, aBytes, w, h, c->dScratch, dPitch);
        YK_HIP(c, hipGetLastError());
    }
    YK_HIP(c, hipMemcpy2DAsync(hostOut, outputImageStride, c->dScratch, dPitch, rowBytes, (size_t)h, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

int yk_decode_output(yk_ctx* c, uint8_t* hostOut, size_t outputImageStride, const uint8_t* hostAlpha, int strideA) {
    return yk_decode_output_impl(c, hostOut, outputImageStride, hostAlpha, strideA, false);
}

int yk_decode_output_alpha(yk_ctx* c, uint8_t* hostOut, size_t outputImageStride) {
    if (!c) return YK_ERR_BAD_ARG;
    YK_DEC_NO_BATCH(c, "yk_decode_output_alpha");
    YK_DEC_NO_WINDOW(c, "yk_decode_output_alpha");
    if (!c->dAlphaValid) return yk_fail(c, YK_ERR_STATE, "yk_decode_alpha first");
    return yk_decode_output_impl(c, hostOut, outputImageStride, nullptr, 0, false, yk_dec_alpha_cur(c));
}

int yk_decode_output_reference_rgba(yk_ctx* c, uint8_t* hostOut, size_t outputImageStride, const uint8_t* hostAlpha, int strideA) {
    if (!c) return YK_ERR_BAD_ARG;
    YK_DEC_NO_BATCH(c, "yk_decode_output_reference_rgba");
    return yk_decode_output_impl(c, hostOut, outputImageStride, hostAlpha, strideA, true);
}

// yk_decode_output_device and yk_decode_output_window_device: the same checks against the size of what is written
static int yk_dec_output_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha, bool window) {
    if (!devOut) return yk_fail(c, YK_ERR_BAD_ARG, "devOut is NULL");
    if (channels != 3 && channels != 4) return yk_fail(c, YK_ERR_BAD_ARG, "channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255)) return yk_fail(c, YK_ERR_BAD_ARG, "alpha must be -1 (the decoded plane) or 0..255");
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    const bool px = window && c->dPxSet;                                      // a pixel window: what is written is dPxW x dPxH of the cover
    const size_t w = (size_t)(px ? c->dPxW : window ? c->dWinW : c->dw), h = (size_t)(px ? c->dPxH : window ? c->dWinH : c->dh);
    if (planeBytes == 0 ? rowBytes < w * channels : (rowBytes < w || planeBytes / h < rowBytes))
        return yk_fail(c, YK_ERR_BAD_ARG, window ? "row or plane pitch too small for the window" : "row or plane pitch too small for the image");
    const bool fromPlane = channels == 4 && alpha < 0;
    if (fromPlane && !c->dAlphaValid) return yk_fail(c, YK_ERR_STATE, "alpha = -1 needs yk_decode_alpha first");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    return yk_dec_detile(c, devOut, rowBytes, planeBytes, channels, fromPlane ? yk_dec_alpha_cur(c) : nullptr, (size_t)c->dw, fromPlane ? 0 : alpha, 0, 0, 0, window);
}

int yk_decode_output_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    YK_DEC_NO_WINDOW(c, "yk_decode_output_device");
    return yk_dec_output_device(c, devOut, rowBytes, planeBytes, channels, alpha, false);
}

int yk_decode_output_window_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    YK_DEC_NO_PREPARED(c, "yk_decode_output_window_device");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_output_window_device");
    return yk_dec_output_device(c, devOut, rowBytes, planeBytes, channels, alpha, c->dWinSet);
}

int yk_decode_output_batch_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!devOut) return yk_refuse(c, YK_ERR_BAD_ARG, "devOut is NULL");
    if (channels != 3 && channels != 4) return yk_refuse(c, YK_ERR_BAD_ARG, "channels must be 3 or 4");
    if (channels == 4 && (alpha < 0 || alpha > 255)) return yk_refuse(c, YK_ERR_BAD_ARG, "alpha must be 0..255 (a batch has no decoded alpha plane)");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_begin_batch first");
    YK_DEC_NO_PREPARED(c, "yk_decode_output_batch_device");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_output_batch_device");
    const size_t w = (size_t)c->dw, h = (size_t)c->dh;
    if (planeBytes == 0 ? rowBytes < w * channels : (rowBytes < w || planeBytes / h < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "row or plane pitch too small for the image");
    if (c->dFrames > 1 && (planeBytes == 0 ? frameBytes / h < rowBytes : frameBytes / (size_t)channels < planeBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "frame stride too small for a frame");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    return yk_dec_detile(c, devOut, rowBytes, planeBytes, channels, nullptr, w, alpha, c->dFrames, frameBytes);
}

// yk_decode_output_batch_device with four channels, alpha from the planes yk_decode_alpha_batch_device left in HBM
int yk_decode_output_batch_alpha_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!devOut) return yk_refuse(c, YK_ERR_BAD_ARG, "devOut is NULL");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_begin_batch first");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_output_batch_alpha_device");
    if (!c->dAlphaValid || !c->dAlphaBatch) return yk_refuse(c, YK_ERR_STATE, "yk_decode_alpha_batch_device first: the batch has no decoded alpha planes");
    const size_t w = (size_t)c->dw, h = (size_t)c->dh;
    if (planeBytes == 0 ? rowBytes < w * 4 : (rowBytes < w || planeBytes / h < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "row or plane pitch too small for the image");
    if (c->dFrames > 1 && (planeBytes == 0 ? frameBytes / h < rowBytes : frameBytes / 4 < planeBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "frame stride too small for a frame");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    return yk_dec_detile(c, devOut, rowBytes, planeBytes, 4, c->dAlpha, w, 0, c->dFrames, frameBytes, c->dAlphaStride);
}

// The window of every frame of a batch with windows (yk_decode_set_batch_windows): frame f's ww x wh pixels at devOut + f * frameBytes, one launch
int yk_decode_output_batch_windows_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!devOut) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_batch_windows_device: devOut is NULL");
    if (channels != 3 && channels != 4) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_batch_windows_device: channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_batch_windows_device: alpha must be -1 (the planes of yk_decode_alpha[_mask]_batch_device) or 0..255");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_batch_windows_device: yk_decode_begin_batch first");
    if (c->dBRectSet) return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_batch_windows_device: rectangles are set on this batch (yk_decode_set_batch_rects): yk_decode_output_resampled_batch_device writes them");
    if (!c->dBWinSet) return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_batch_windows_device: no windows are set on this batch (yk_decode_set_batch_windows)");
    const bool fromPlanes = channels == 4 && alpha < 0;
    if (fromPlanes && (!c->dAlphaValid || !c->dAlphaBatch))
        return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_batch_windows_device: alpha = -1 needs yk_decode_alpha_batch_device first: the batch has no decoded alpha planes");
    const bool px = c->dPxSet;                                                // pixel windows: dPxW x dPxH of every frame's cover is written
    const size_t w = (size_t)(px ? c->dPxW : c->dBWinW), h = (size_t)(px ? c->dPxH : c->dBWinH);
    if (planeBytes == 0 ? rowBytes < w * channels : (rowBytes < w || planeBytes / h < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_batch_windows_device: row or plane pitch too small for the window");
    if (c->dFrames > 1 && (planeBytes == 0 ? frameBytes / h < rowBytes : frameBytes / (size_t)channels < planeBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_batch_windows_device: frame stride too small for a window");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    YkDetileArgs a;
    a.planes = c->dB.planes; a.planeSize = c->dPlaneSize;
    a.alpha = fromPlanes ? (const uint8_t*)c->dAlpha : nullptr; a.strideA = (size_t)c->dw; a.alphaConst = (uint32_t)((fromPlanes ? 0 : alpha) & 255) * 0x01010101u;
    a.out = devOut; a.rowBytes = rowBytes; a.planeBytes = planeBytes;
    a.tileW = (uint32_t)(c->dw >> 3); a.nTiles = (uint32_t)(c->dBWinW >> 3) * (uint32_t)(c->dBWinH >> 3);
    const uint32_t wtW = (uint32_t)(c->dBWinW >> 3);
    const size_t pf = c->dStride.planes, af = fromPlanes ? c->dAlphaStride : 0;
    const DWinRect* wins = yk_dec_bwin_tab(c);
    const bool planar = planeBytes > 0;
    const int N = c->dFrames;
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_DETILE); if (rc) return rc; }
    if (px) {                                                                 // the covers' tiles, each frame clipped to its window; the offsets follow the rectangles
        const int* off = c->dBWinTab.p + 4 * (size_t)N;
        const unsigned gx = (a.nTiles + YK_DT_TILES - 1) / YK_DT_TILES;
        const int pw = c->dPxW, ph = c->dPxH;
        yk_dt_each(channels, planar, fromPlanes, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((yk_dec_detile_batch_win_px_kernel<T::c, T::planar, T::asrc>), dim3(gx, (unsigned)N), dim3(YK_DT_THREADS), 0, c->stream, a, wins, off, wtW, pw, ph,
                               pf, frameBytes, af);
        });
        YK_HIP(c, hipGetLastError());
        return yk_stage_end(c, YK_STAGE_DEC_DETILE);
    }
    if (channels == 3)   { if (planar) yk_dt_launch_batch_win<3, true, YK_DT_ALPHA_NONE>(a, c->stream, N, wins, wtW, pf, frameBytes, 0); else yk_dt_launch_batch_win<3, false, YK_DT_ALPHA_NONE>(a, c->stream, N, wins, wtW, pf, frameBytes, 0); }
    else if (fromPlanes) { if (planar) yk_dt_launch_batch_win<4, true, YK_DT_ALPHA_PLANE>(a, c->stream, N, wins, wtW, pf, frameBytes, af); else yk_dt_launch_batch_win<4, false, YK_DT_ALPHA_PLANE>(a, c->stream, N, wins, wtW, pf, frameBytes, af); }
    else                 { if (planar) yk_dt_launch_batch_win<4, true, YK_DT_ALPHA_CONST>(a, c->stream, N, wins, wtW, pf, frameBytes, 0); else yk_dt_launch_batch_win<4, false, YK_DT_ALPHA_CONST>(a, c->stream, N, wins, wtW, pf, frameBytes, 0); }
    YK_HIP(c, hipGetLastError());
    return yk_stage_end(c, YK_STAGE_DEC_DETILE);
}

// ---- normalised outputs (include/yaik_hip.h): both entry points, every check before anything is queued, then one launch ------------
static int yk_dec_output_norm(yk_ctx* c, const char* name, const yk_norm* nrm, int mirrorOne, const uint8_t* mirrorTab, void* devOut, size_t rowBytes, size_t planeBytes,
                              size_t frameBytes, int channels, int alpha, bool batch) {
    auto refuse = [&](int code, const char* what) { return yk_refuse(c, code, (std::string(name) + ": " + what).c_str()); };
    if (!nrm) return refuse(YK_ERR_BAD_ARG, "norm is NULL");
    if (!devOut) return refuse(YK_ERR_BAD_ARG, "devOut is NULL");
    if (nrm->dtype != YK_ELEM_F16 && nrm->dtype != YK_ELEM_BF16 && nrm->dtype != YK_ELEM_F32) return refuse(YK_ERR_BAD_ARG, "dtype must be YK_ELEM_F16, YK_ELEM_BF16 or YK_ELEM_F32");
    for (int k = 0; k < 4; k++)
        if (!yk_norm_param_ok(nrm->scale[k]) || !yk_norm_param_ok(nrm->bias[k]))
            return refuse(YK_ERR_BAD_ARG, "every scale and bias must be finite and 0 or of magnitude in [2^-100, 2^100]");
    if (channels != 3 && channels != 4) return refuse(YK_ERR_BAD_ARG, "channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255)) return refuse(YK_ERR_BAD_ARG, "alpha must be -1 (the decoded plane) or 0..255");
    const size_t es = nrm->dtype == YK_ELEM_F32 ? 4 : 2;
    if (((uintptr_t)devOut | rowBytes | planeBytes | (batch ? frameBytes : 0)) & (es - 1)) return refuse(YK_ERR_BAD_ARG, "devOut and every pitch must be multiples of the element size");
    if (!yk_dec_begun(c)) return refuse(YK_ERR_STATE, batch ? "yk_decode_begin_batch first" : "yk_decode_begin first");
    if (c->dPrepared) return refuse(YK_ERR_STATE, "this image is prepared for windows (yk_decode_prepare_device), which have no normalised output");
    if (c->dBRectSet) return refuse(YK_ERR_STATE, "rectangles are set on this batch (yk_decode_set_batch_rects): yk_decode_output_resampled_batch_device writes them");
    if (!batch && c->dBWinSet) return refuse(YK_ERR_STATE, "windows are set on this batch (yk_decode_set_batch_windows): yk_decode_output_norm_batch_device writes them");
    if (batch && c->dWinSet) return refuse(YK_ERR_STATE, "a window is set on this image (yk_decode_set_window): yk_decode_output_norm_device writes it");
    const bool fromPlane = channels == 4 && alpha < 0;
    if (fromPlane && (!c->dAlphaValid || (batch && !c->dAlphaBatch)))
        return refuse(YK_ERR_STATE, batch ? "alpha = -1 needs yk_decode_alpha_batch_device first: the batch has no decoded alpha planes" : "alpha = -1 needs yk_decode_alpha first");
    // what is written, and the cover whose tiles the kernel walks
    const bool bwin = batch && c->dBWinSet, win = !batch && c->dWinSet, px = (bwin || win) && c->dPxSet;
    const int cw = bwin ? c->dBWinW : win ? c->dWinW : c->dw, ch = bwin ? c->dBWinH : win ? c->dWinH : c->dh;
    const size_t w = (size_t)(px ? c->dPxW : cw), h = (size_t)(px ? c->dPxH : ch);
    if (planeBytes == 0 ? rowBytes / es < w * (size_t)channels : (rowBytes / es < w || planeBytes / h < rowBytes))
        return refuse(YK_ERR_BAD_ARG, "row or plane pitch too small for what is written");
    const int N = batch ? c->dFrames : 1;
    if (N > 1 && (planeBytes == 0 ? frameBytes / h < rowBytes : frameBytes / (size_t)channels < planeBytes)) return refuse(YK_ERR_BAD_ARG, "frame stride too small for a frame");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    const uint32_t* devMirror = nullptr;
    if (batch && mirrorTab) {                                                 // the flags through the pinned ring, behind the kernels of an earlier call
        YK_HIP(c, c->dNormTab.reserve(c->stream, 1024));
        int slot; void* host;
        { const int rc = yk_dec_table_host(c, (size_t)N * sizeof(uint32_t), &slot, &host); if (rc) return rc; }
        for (int f = 0; f < N; f++) static_cast<uint32_t*>(host)[f] = mirrorTab[f] ? 1u : 0u;
        { const int rc = yk_dec_table_upload(c, slot, c->dNormTab.p, (size_t)N * sizeof(uint32_t)); if (rc) return rc; }
        devMirror = c->dNormTab.p;
    }
    YkDetileArgs a;
    a.planes = batch ? c->dB.planes : yk_dec_frame(c, c->dCur).planes; a.planeSize = c->dPlaneSize;
    a.alpha = fromPlane ? (batch ? (const uint8_t*)c->dAlpha : yk_dec_alpha_cur(c)) : nullptr; a.strideA = (size_t)c->dw;
    a.alphaConst = (uint32_t)((fromPlane ? 0 : alpha) & 255) * 0x01010101u;
    a.out = static_cast<uint8_t*>(devOut); a.rowBytes = rowBytes; a.planeBytes = planeBytes;
    a.tileW = (uint32_t)(c->dw >> 3); a.nTiles = (uint32_t)(cw >> 3) * (uint32_t)(ch >> 3);
    YkDetileNorm nm;
    for (int k = 0; k < 4; k++) { nm.scale[k] = nrm->scale[k]; nm.bias[k] = nrm->bias[k]; }
    nm.cx0 = win ? (uint32_t)c->dWinX : 0; nm.cy0 = win ? (uint32_t)c->dWinY : 0;
    nm.dx = win && px ? c->dPxX - c->dWinX : 0; nm.dy = win && px ? c->dPxY - c->dWinY : 0;
    nm.ww = (int)w; nm.wh = (int)h; nm.mirror = !batch && mirrorOne ? 1u : 0u;
    const DWinRect* wins = bwin ? yk_dec_bwin_tab(c) : nullptr;
    const int* off = bwin && px ? c->dBWinTab.p + 4 * (size_t)N : nullptr;
    const size_t pf = batch ? c->dStride.planes : 0, af = batch && fromPlane ? c->dAlphaStride : 0;
    const bool planar = planeBytes > 0;
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_DETILE); if (rc) return rc; }
    if (nrm->dtype == YK_ELEM_F16) yk_dn_launch<YK_ELEM_F16>(a, nm, c->stream, channels, planar, fromPlane, N, wins, off, devMirror, (uint32_t)(cw >> 3), pf, frameBytes, af);
    else if (nrm->dtype == YK_ELEM_BF16) yk_dn_launch<YK_ELEM_BF16>(a, nm, c->stream, channels, planar, fromPlane, N, wins, off, devMirror, (uint32_t)(cw >> 3), pf, frameBytes, af);
    else yk_dn_launch<YK_ELEM_F32>(a, nm, c->stream, channels, planar, fromPlane, N, wins, off, devMirror, (uint32_t)(cw >> 3), pf, frameBytes, af);
    YK_HIP(c, hipGetLastError());
    return yk_stage_end(c, YK_STAGE_DEC_DETILE);
}
int yk_decode_output_norm_device(yk_ctx* c, const yk_norm* norm, int mirror, void* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    return yk_dec_output_norm(c, "yk_decode_output_norm_device", norm, mirror, nullptr, devOut, rowBytes, planeBytes, 0, channels, alpha, false);
}
int yk_decode_output_norm_batch_device(yk_ctx* c, const yk_norm* norm, const uint8_t* mirror, void* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes,
                                       int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    return yk_dec_output_norm(c, "yk_decode_output_norm_batch_device", norm, 0, mirror, devOut, rowBytes, planeBytes, frameBytes, channels, alpha, true);
}

// ---- resampled outputs (include/yaik_hip.h): both entry points, every check before anything is queued (the table upload included),
// then the nine words per frame through the pinned ring and one launch
static int yk_dec_output_resampled(yk_ctx* c, const char* name, const int* rectOne, const yk_norm* nrm, int mirrorOne, const uint8_t* mirrorTab, void* devOut, int ow, int oh,
                                   size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha, bool batch) {
    auto refuse = [&](int code, const char* what) { return yk_refuse(c, code, (std::string(name) + ": " + what).c_str()); };
    if (!devOut) return refuse(YK_ERR_BAD_ARG, "devOut is NULL");
    if (nrm) {
        if (nrm->dtype != YK_ELEM_F16 && nrm->dtype != YK_ELEM_BF16 && nrm->dtype != YK_ELEM_F32) return refuse(YK_ERR_BAD_ARG, "dtype must be YK_ELEM_F16, YK_ELEM_BF16 or YK_ELEM_F32");
        for (int k = 0; k < 4; k++)
            if (!yk_norm_param_ok(nrm->scale[k]) || !yk_norm_param_ok(nrm->bias[k]))
                return refuse(YK_ERR_BAD_ARG, "every scale and bias must be finite and 0 or of magnitude in [2^-100, 2^100]");
    }
    if (channels != 3 && channels != 4) return refuse(YK_ERR_BAD_ARG, "channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255)) return refuse(YK_ERR_BAD_ARG, "alpha must be -1 (the decoded plane) or 0..255");
    if (!yk_rs_size_ok(ow, oh)) return refuse(YK_ERR_BAD_ARG, "the output size must be 1..16384 on both sides");
    const size_t es = !nrm ? 1 : nrm->dtype == YK_ELEM_F32 ? 4 : 2;
    if (((uintptr_t)devOut | rowBytes | planeBytes | (batch ? frameBytes : 0)) & (es - 1)) return refuse(YK_ERR_BAD_ARG, "devOut and every pitch must be multiples of the element size");
    if (!yk_dec_begun(c)) return refuse(YK_ERR_STATE, batch ? "yk_decode_begin_batch first" : "yk_decode_begin first");
    if (c->dPrepared) return refuse(YK_ERR_STATE, "this image is prepared for windows (yk_decode_prepare_device), which have no resampled output");
    if (!batch && c->dBRectSet) return refuse(YK_ERR_STATE, "rectangles are set on this batch (yk_decode_set_batch_rects): yk_decode_output_resampled_batch_device writes them");
    if (!batch && c->dBWinSet) return refuse(YK_ERR_STATE, "windows are set on this batch (yk_decode_set_batch_windows), which have no resampled output");
    if (batch && c->dBWinSet && !c->dBRectSet) return refuse(YK_ERR_STATE, "windows are set on this batch (yk_decode_set_batch_windows): set rectangles (yk_decode_set_batch_rects) or neither");
    if (batch && c->dWinSet) return refuse(YK_ERR_STATE, "a window is set on this image (yk_decode_set_window): yk_decode_output_resampled_device reads it");
    const bool fromPlane = channels == 4 && alpha < 0;
    if (fromPlane && (!c->dAlphaValid || (batch && !c->dAlphaBatch)))
        return refuse(YK_ERR_STATE, batch ? "alpha = -1 needs yk_decode_alpha_batch_device first: the batch has no decoded alpha planes" : "alpha = -1 needs yk_decode_alpha first");
    // the single call's rectangle: inside the window (the pixel window if one is set), which is all the planes hold
    int one[4] = { 0, 0, c->dw, c->dh };
    if (!batch) {
        if (c->dWinSet) { const bool px = c->dPxSet; one[0] = px ? c->dPxX : c->dWinX; one[1] = px ? c->dPxY : c->dWinY; one[2] = px ? c->dPxW : c->dWinW; one[3] = px ? c->dPxH : c->dWinH; }
        if (rectOne) {
            const int bx0 = one[0], by0 = one[1], bw = one[2], bh = one[3];
            if (!yk_rs_src_ok(rectOne[0], rectOne[1], rectOne[2], rectOne[3], c->dw, c->dh))
                return refuse(YK_ERR_BAD_ARG, "x0, y0 >= 0, 1 <= sw, sh <= 16384 and the rectangle inside the image");
            if (rectOne[0] < bx0 || rectOne[1] < by0 || rectOne[0] - bx0 > bw - rectOne[2] || rectOne[1] - by0 > bh - rectOne[3])
                return refuse(YK_ERR_BAD_ARG, "the rectangle must lie inside the window set on this image");
            for (int k = 0; k < 4; k++) one[k] = rectOne[k];
        }
    }
    const int N = batch ? c->dFrames : 1;
    if (!(batch && c->dBRectSet) && (one[2] > YK_RS_MAX || one[3] > YK_RS_MAX)) return refuse(YK_ERR_BAD_ARG, "the source rectangle must be 16384 pixels or less on both sides");
    const size_t w = (size_t)ow, h = (size_t)oh;
    if (planeBytes == 0 ? rowBytes / es < w * (size_t)channels : (rowBytes / es < w || planeBytes / h < rowBytes))
        return refuse(YK_ERR_BAD_ARG, "row or plane pitch too small for what is written");
    if (N > 1 && (planeBytes == 0 ? frameBytes / h < rowBytes : frameBytes / (size_t)channels < planeBytes)) return refuse(YK_ERR_BAD_ARG, "frame stride too small for a frame");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    YK_HIP(c, c->dRsTab.reserve(c->stream, (size_t)1024 * YK_RS_WORDS));        // allocated once: a queued earlier call has read its words before this call's copy runs
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, (size_t)N * YK_RS_WORDS * sizeof(int), &slot, &host); if (rc) return rc; }
    for (int f = 0; f < N; f++) {
        const int* r = batch && c->dBRectSet ? &c->dBRects[4 * (size_t)f] : one;
        yk_rs_words(r[0], r[1], r[2], r[3], ow, oh, batch ? (mirrorTab && mirrorTab[f]) : mirrorOne != 0, static_cast<int*>(host) + (size_t)f * YK_RS_WORDS);
    }
    { const int rc = yk_dec_table_upload(c, slot, c->dRsTab.p, (size_t)N * YK_RS_WORDS * sizeof(int)); if (rc) return rc; }
    YkResampleArgs a;
    a.planes = batch ? c->dB.planes : yk_dec_frame(c, c->dCur).planes; a.planeSize = c->dPlaneSize; a.planesFrame = batch ? c->dStride.planes : 0;
    a.alpha = fromPlane ? (batch ? (const uint8_t*)c->dAlpha : yk_dec_alpha_cur(c)) : nullptr; a.strideA = (size_t)c->dw; a.alphaFrame = batch && fromPlane ? c->dAlphaStride : 0;
    a.alphaConst = (uint32_t)((fromPlane ? 0 : alpha) & 255);
    a.out = static_cast<uint8_t*>(devOut); a.rowBytes = rowBytes; a.planeBytes = planeBytes; a.outFrame = batch ? frameBytes : 0;
    a.tileW = (uint32_t)(c->dw >> 3); a.nbx = ((uint32_t)ow + YK_RS_BW - 1) / YK_RS_BW; a.ow = ow; a.oh = oh;
    for (int k = 0; k < 4; k++) { a.scale[k] = nrm ? nrm->scale[k] : 1.0f; a.bias[k] = nrm ? nrm->bias[k] : 0.0f; }
    a.tab = c->dRsTab.p;
    const bool planar = planeBytes > 0;
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_DETILE); if (rc) return rc; }
    if (!nrm) yk_rs_launch<0>(a, c->stream, channels, planar, fromPlane, N);
    else if (nrm->dtype == YK_ELEM_F16) yk_rs_launch<YK_ELEM_F16>(a, c->stream, channels, planar, fromPlane, N);
    else if (nrm->dtype == YK_ELEM_BF16) yk_rs_launch<YK_ELEM_BF16>(a, c->stream, channels, planar, fromPlane, N);
    else yk_rs_launch<YK_ELEM_F32>(a, c->stream, channels, planar, fromPlane, N);
    YK_HIP(c, hipGetLastError());
    return yk_stage_end(c, YK_STAGE_DEC_DETILE);
}
int yk_decode_output_resampled_batch_device(yk_ctx* c, const yk_norm* norm, const uint8_t* mirror, void* devOut, int ow, int oh, size_t rowBytes, size_t planeBytes,
                                            size_t frameBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    return yk_dec_output_resampled(c, "yk_decode_output_resampled_batch_device", nullptr, norm, 0, mirror, devOut, ow, oh, rowBytes, planeBytes, frameBytes, channels, alpha, true);
}
int yk_decode_output_resampled_device(yk_ctx* c, const int* rect, const yk_norm* norm, int mirror, void* devOut, int ow, int oh, size_t rowBytes, size_t planeBytes, int channels,
                                      int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    return yk_dec_output_resampled(c, "yk_decode_output_resampled_device", rect, norm, mirror, nullptr, devOut, ow, oh, rowBytes, planeBytes, 0, channels, alpha, false);
}

// ---- outputs at reduced resolution (include/yaik_hip.h): level 0 is the full-size call, 1..3 the box means of 2x2, 4x4, 8x8 ----------
int yk_decode_output_scaled_device(yk_ctx* c, int level, uint8_t* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    if (level < 0 || level > 3) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_device: level must be 0..3");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_scaled_device: yk_decode_begin first");
    if (c->dPrepared)
        return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_scaled_device: this image is prepared for windows (yk_decode_prepare_device); yk_decode_render_windows_scaled_device reads it");
    if (level == 0) return yk_decode_output_window_device(c, devOut, rowBytes, planeBytes, channels, alpha);
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_output_scaled_device");
    if (c->dWinSet && c->dPxSet)
        return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_scaled_device: a pixel window is set on this decode (yk_decode_set_window_px) and its boxes would not be aligned; yk_decode_output_window_device writes it at full size");
    if (!devOut) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_device: devOut is NULL");
    if (channels != 3 && channels != 4) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_device: channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255)) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_device: alpha must be -1 (the decoded plane) or 0..255");
    const bool window = c->dWinSet;
    const size_t w = (size_t)(window ? c->dWinW : c->dw) >> level, h = (size_t)(window ? c->dWinH : c->dh) >> level;
    if (planeBytes == 0 ? rowBytes < w * channels : (rowBytes < w || planeBytes / h < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_device: row or plane pitch too small for the reduced image or window");
    const bool fromPlane = channels == 4 && alpha < 0;
    if (fromPlane && !c->dAlphaValid) return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_scaled_device: alpha = -1 needs yk_decode_alpha first");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    return yk_dec_detile_scaled(c, level, devOut, rowBytes, planeBytes, channels, fromPlane ? yk_dec_alpha_cur(c) : nullptr, (size_t)c->dw, fromPlane ? 0 : alpha, 0, 0, 0, window);
}

int yk_decode_output_scaled_batch_device(yk_ctx* c, int level, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    if (level < 0 || level > 3) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_batch_device: level must be 0..3");
    if (channels != 3 && channels != 4) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_batch_device: channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_batch_device: alpha must be -1 (the planes of yk_decode_alpha[_mask]_batch_device) or 0..255");
    const bool fromPlanes = channels == 4 && alpha < 0;
    if (level == 0) {
        if (fromPlanes) return yk_decode_output_batch_alpha_device(c, devOut, rowBytes, planeBytes, frameBytes);
        return yk_decode_output_batch_device(c, devOut, rowBytes, planeBytes, frameBytes, channels, channels == 4 ? alpha : 255);
    }
    if (!devOut) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_batch_device: devOut is NULL");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_scaled_batch_device: yk_decode_begin_batch first");
    YK_DEC_NO_PREPARED(c, "yk_decode_output_scaled_batch_device");
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_output_scaled_batch_device");
    if (fromPlanes && (!c->dAlphaValid || !c->dAlphaBatch))
        return yk_refuse(c, YK_ERR_STATE, "yk_decode_output_scaled_batch_device: alpha = -1 needs yk_decode_alpha_batch_device first: the batch has no decoded alpha planes");
    const size_t w = (size_t)c->dw >> level, h = (size_t)c->dh >> level;
    if (planeBytes == 0 ? rowBytes < w * channels : (rowBytes < w || planeBytes / h < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_batch_device: row or plane pitch too small for the reduced image");
    if (c->dFrames > 1 && (planeBytes == 0 ? frameBytes / h < rowBytes : frameBytes / (size_t)channels < planeBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_output_scaled_batch_device: frame stride too small for a reduced frame");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    return yk_dec_detile_scaled(c, level, devOut, rowBytes, planeBytes, channels, fromPlanes ? c->dAlpha : nullptr, (size_t)c->dw, fromPlanes ? 0 : alpha, c->dFrames, frameBytes,
                                fromPlanes ? c->dAlphaStride : 0);
}

// ---- a mip chain in one call (include/yaik_hip.h): levels firstLevel .. firstLevel + nLevels - 1, the planes read once ---------------
int yk_decode_mip_levels(int w, int h) {
    if (w < 8 || h < 8 || (w & 7) || (h & 7) || w > 32760 || h > 32760) return YK_ERR_BAD_ARG;
    int n = 0;
    for (int m = w < h ? w : h; m; m >>= 1) n++;
    return n;                                                                   // floor(log2(min(w, h))) + 1
}

// both entry points: every check against the level's own size, then at most two launches inside one YK_STAGE_DEC_DETILE interval
static int yk_dec_mipchain(yk_ctx* c, const char* name, int firstLevel, int nLevels, const yk_mip_level* levels, int channels, int alpha, bool batch) {
    auto refuse = [&](int code, const char* what) { return yk_refuse(c, code, (std::string(name) + ": " + what).c_str()); };
    if (!yk_dec_begun(c)) return refuse(YK_ERR_STATE, batch ? "yk_decode_begin_batch first" : "yk_decode_begin first");
    if (c->dPrepared) return refuse(YK_ERR_STATE, "this image is prepared for windows (yk_decode_prepare_device) and windows have no chain");
    if (!batch && c->dWinSet) return refuse(YK_ERR_STATE, "a window is set on this decode (yk_decode_set_window) and windows have no chain");
    if (c->dBRectSet) return refuse(YK_ERR_STATE, "rectangles are set on this batch (yk_decode_set_batch_rects) and rectangles have no chain");
    if (c->dBWinSet) return refuse(YK_ERR_STATE, "windows are set on this batch (yk_decode_set_batch_windows) and windows have no chain");
    const int total = yk_decode_mip_levels(c->dw, c->dh);
    if (firstLevel < 0 || nLevels < 1 || nLevels > YK_MIP_MAX_LEVELS || firstLevel > total - nLevels)
        return refuse(YK_ERR_BAD_ARG, "firstLevel .. firstLevel + nLevels - 1 must lie inside the image's levels (yk_decode_mip_levels)");
    if (!levels) return refuse(YK_ERR_BAD_ARG, "levels is NULL");
    if (channels != 3 && channels != 4) return refuse(YK_ERR_BAD_ARG, "channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255)) return refuse(YK_ERR_BAD_ARG, "alpha must be -1 (the decoded alpha) or 0..255");
    const bool planar = levels[0].planeBytes > 0;
    const int nFrames = batch ? c->dFrames : 1;
    for (int i = 0; i < nLevels; i++) {
        const yk_mip_level& L = levels[i];
        const size_t w = (size_t)c->dw >> (firstLevel + i), h = (size_t)c->dh >> (firstLevel + i);
        if (!L.devOut) return refuse(YK_ERR_BAD_ARG, "a level's devOut is NULL");
        if ((L.planeBytes > 0) != planar) return refuse(YK_ERR_BAD_ARG, "the levels of one call are all HWC (planeBytes == 0) or all CHW");
        if (!planar ? L.rowBytes < w * channels : (L.rowBytes < w || L.planeBytes / h < L.rowBytes))
            return refuse(YK_ERR_BAD_ARG, "row or plane pitch too small for a level");
        if (nFrames > 1 && (!planar ? L.frameBytes / h < L.rowBytes : L.frameBytes / (size_t)channels < L.planeBytes))
            return refuse(YK_ERR_BAD_ARG, "frame stride too small for a level's frame");
    }
    const bool fromPlane = channels == 4 && alpha < 0;
    if (fromPlane && batch && (!c->dAlphaValid || !c->dAlphaBatch))
        return refuse(YK_ERR_STATE, "alpha = -1 needs yk_decode_alpha_batch_device first: the batch has no decoded alpha planes");
    if (fromPlane && !c->dAlphaValid) return refuse(YK_ERR_STATE, "alpha = -1 needs yk_decode_alpha first");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    const int lastLevel = firstLevel + nLevels - 1;
    YkMipArgs a = {};
    YkMipTailArgs t = {};
    a.planes = yk_dec_frame(c, batch ? 0 : c->dCur).planes; a.planeSize = c->dPlaneSize; a.planesFrame = c->dStride.planes;
    a.alpha = fromPlane ? (batch ? (const uint8_t*)c->dAlpha : yk_dec_alpha_cur(c)) : nullptr; a.strideA = (size_t)c->dw; a.alphaFrame = fromPlane && batch ? c->dAlphaStride : 0;
    a.alphaConst = (uint32_t)((fromPlane ? 0 : alpha) & 255) * 0x01010101u;
    a.w = (uint32_t)c->dw; a.h = (uint32_t)c->dh; a.nbx = (a.w + 63) >> 6;
    a.high = lastLevel >= 4; a.sbx = a.w >> 6; a.sby = a.h >> 6;
    t.first = firstLevel > 7 ? firstLevel : 7; t.last = lastLevel;
    if (lastLevel >= 7) {
        { const int rc = yk_dec_scratch(c, (size_t)nFrames * a.sbx * a.sby * 16); if (rc) return rc; }
        a.sums = reinterpret_cast<uint32_t*>(c->dScratch.p);
        t.sums = a.sums; t.sbx = a.sbx; t.sby = a.sby; t.w = a.w; t.h = a.h; t.alphaConst = a.alphaConst;
    }
    for (int i = 0; i < nLevels; i++) {
        const YkMipDst d = { levels[i].devOut, levels[i].rowBytes, levels[i].planeBytes, levels[i].frameBytes };
        if (firstLevel + i < 7) a.lv[firstLevel + i] = d; else t.lv[firstLevel + i - 7] = d;
    }
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_DETILE); if (rc) return rc; }
    const unsigned nf = (unsigned)nFrames;
    if (channels == 3)  { if (planar) yk_mip_launch<3, true, YK_DT_ALPHA_NONE>(a, t, c->stream, nf); else yk_mip_launch<3, false, YK_DT_ALPHA_NONE>(a, t, c->stream, nf); }
    else if (fromPlane) { if (planar) yk_mip_launch<4, true, YK_DT_ALPHA_PLANE>(a, t, c->stream, nf); else yk_mip_launch<4, false, YK_DT_ALPHA_PLANE>(a, t, c->stream, nf); }
    else                { if (planar) yk_mip_launch<4, true, YK_DT_ALPHA_CONST>(a, t, c->stream, nf); else yk_mip_launch<4, false, YK_DT_ALPHA_CONST>(a, t, c->stream, nf); }
    YK_HIP(c, hipGetLastError());
    return yk_stage_end(c, YK_STAGE_DEC_DETILE);
}

int yk_decode_output_mipchain_device(yk_ctx* c, int firstLevel, int nLevels, const yk_mip_level* levels, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    return yk_dec_mipchain(c, "yk_decode_output_mipchain_device", firstLevel, nLevels, levels, channels, alpha, false);
}

int yk_decode_output_mipchain_batch_device(yk_ctx* c, int firstLevel, int nLevels, const yk_mip_level* levels, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    return yk_dec_mipchain(c, "yk_decode_output_mipchain_batch_device", firstLevel, nLevels, levels, channels, alpha, true);
}

// ---- round-trip quality: the decode against a source in HBM (kernels and the read-back: yk_quality.hip) ----
// the checks the three entry points share; batch: every frame (else the selected one)
static int yk_dec_compare_common(yk_ctx* c, int channels, const void* out, bool batch) {
    if (!out) return yk_refuse(c, YK_ERR_BAD_ARG, "out is NULL");
    if (channels != 3 && channels != 4) return yk_refuse(c, YK_ERR_BAD_ARG, "channels must be 3 or 4");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, batch ? "yk_decode_begin_batch first" : "yk_decode_begin first");
    YK_DEC_NO_WINDOW(c, "yk_decode_compare_*");
    if (channels == 4 && !c->dAlphaValid)
        return yk_refuse(c, YK_ERR_STATE, "channels = 4 needs the decoded alpha: yk_decode_alpha or yk_decode_alpha_batch_device first");
    return YK_OK;
}
static int yk_dec_compare_u8(yk_ctx* c, const uint8_t* devSrc, size_t rowBytes, size_t planeBytes, size_t frameBytes, int srcChannels, int channels,
                             yk_quality* out, uint32_t* devTileSse, bool batch) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!devSrc) return yk_refuse(c, YK_ERR_BAD_ARG, "devSrc is NULL");
    { const int rc = yk_dec_compare_common(c, channels, out, batch); if (rc) return rc; }
    if ((srcChannels != 3 && srcChannels != 4) || srcChannels < channels)
        return yk_refuse(c, YK_ERR_BAD_ARG, "srcChannels must be 3 or 4 and at least channels");
    const size_t w = (size_t)c->dw, h = (size_t)c->dh;
    if (planeBytes == 0 ? rowBytes / (size_t)srcChannels < w : (rowBytes < w || planeBytes / h < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "row or plane pitch too small for the image");
    const int nFrames = batch ? c->dFrames : 1;
    if (nFrames > 1 && (planeBytes == 0 ? frameBytes / h < rowBytes : frameBytes / (size_t)channels < planeBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "frame stride too small for a frame");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    const YkQualitySrc q = { devSrc, rowBytes, planeBytes, srcChannels, nullptr, 0, nFrames > 1 ? frameBytes : 0 };
    return yk_quality_compare(c, q, batch ? 0 : c->dCur, nFrames, channels, out, devTileSse);
}

int yk_decode_compare_device(yk_ctx* c, const uint8_t* devSrc, size_t rowBytes, size_t planeBytes, int srcChannels, int channels, yk_quality* out,
                             uint32_t* devTileSse) {
    return yk_dec_compare_u8(c, devSrc, rowBytes, planeBytes, 0, srcChannels, channels, out, devTileSse, false);
}

int yk_decode_compare_batch_device(yk_ctx* c, const uint8_t* devSrc, size_t rowBytes, size_t planeBytes, size_t frameBytes, int srcChannels, int channels,
                                   yk_quality* out, uint32_t* devTileSse) {
    return yk_dec_compare_u8(c, devSrc, rowBytes, planeBytes, frameBytes, srcChannels, channels, out, devTileSse, true);
}

int yk_decode_compare_planes_device(yk_ctx* c, const int32_t* const frame0Planes[4], int strideElems, size_t frameStrideElems, int channels, yk_quality* out,
                                    uint32_t* devTileSse) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!frame0Planes) return yk_refuse(c, YK_ERR_BAD_ARG, "frame0Planes is NULL");
    { const int rc = yk_dec_compare_common(c, channels, out, true); if (rc) return rc; }
    for (int k = 0; k < channels; k++) if (!frame0Planes[k]) return yk_refuse(c, YK_ERR_BAD_ARG, "a plane the comparison needs is NULL");
    if (strideElems < c->dw) return yk_refuse(c, YK_ERR_BAD_ARG, "strideElems is smaller than the width");
    YK_HIP(c, hipSetDevice(c->device));
    { const int rcs = yk_dec_settle(c); if (rcs) return rcs; }
    const YkQualitySrc q = { nullptr, 0, 0, 0, frame0Planes, (size_t)strideElems, c->dFrames > 1 ? frameStrideElems : 0 };
    return yk_quality_compare(c, q, 0, c->dFrames, channels, out, devTileSse);
}

const uint8_t* yk_decode_planes_device(yk_ctx* c, size_t* planeSize) {
    if (!c || !yk_dec_begun(c)) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess || yk_dec_settle(c) != YK_OK) return nullptr;
    if (planeSize) *planeSize = c->dPlaneSize;
    return yk_dec_frame(c).planes;
}

int yk_decode_tile4x4_planes(yk_ctx* c, uint8_t* hostOut, size_t cap) {     // the three planes of tile4x4Mask (planes 1, 2 are meaningful once split)
    if (!c || !hostOut) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    if (cap < 3 * c->dTile4Size) return yk_fail(c, YK_ERR_RANGE, "tile4x4 buffer too small");
    YK_HIP(c, hipSetDevice(c->device));
    YK_HIP(c, hipMemcpyAsync(hostOut, yk_dec_frame(c).tile4, 3 * c->dTile4Size, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

int yk_decode_tile4x4(yk_ctx* c, uint8_t* hostOut, size_t cap) {
    if (!c || !hostOut) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    if (cap < c->dTile4Size) return yk_fail(c, YK_ERR_RANGE, "tile4x4 buffer too small");
    YK_HIP(c, hipSetDevice(c->device));
    YK_HIP(c, hipMemcpyAsync(hostOut, yk_dec_frame(c).tile4, c->dTile4Size, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

// ---- many windows of one image: the map-sized work once, 64x64 blocks rendered on demand (include/yaik_hip.h) ------------------
int yk_decode_prepare_device(yk_ctx* c, int nPasses, const int* tileShiftX, const int* tileShiftY, const uint8_t* const* devBitmap, const size_t* bitmapBytes,
                             const uint8_t* const* devRgb, const size_t* rgbBytes, int remapRange, const uint8_t* devType, size_t typeBytes, const uint8_t* devPix,
                             size_t pixBytes, int compressionRange) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_prepare_device: yk_decode_begin first");
    if (c->dPrepared) return yk_refuse(c, YK_ERR_STATE, "yk_decode_prepare_device: this image is prepared already; yk_decode_begin starts the next one");
    if (c->dBatchBegun || c->dFrames > 1) return yk_refuse(c, YK_ERR_STATE, "yk_decode_prepare_device: a single image (yk_decode_begin) is prepared, not a batch");
    if (c->dWinSet) return yk_refuse(c, YK_ERR_STATE, "yk_decode_prepare_device: a window is set on this decode (yk_decode_set_window); prepare takes the whole image");
    if (c->dChunkSeen) return yk_refuse(c, YK_ERR_STATE, "yk_decode_prepare_device: a chunk of this image has been decoded already; prepare right after yk_decode_begin");
    if (nPasses < 0 || (nPasses && (!tileShiftX || !tileShiftY || !devBitmap || !bitmapBytes || !devRgb || !rgbBytes)))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_prepare_device: negative pass count or NULL table");
    if (nPasses > 7) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_prepare_device takes at most 7 gradient passes; decode such an image window by window (yk_decode_set_window)");
    const int w = c->dw, h = c->dh, latW = w / 4 + 1, tilesW = w >> 3;
    size_t need[7] = {};
    for (int p = 0; p < nPasses; p++) {
        if (!(need[p] = yk_dpass_bytes(tileShiftX[p], tileShiftY[p], w, h))) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_prepare_device: unsupported tile format");
        if (!devBitmap[p] || (rgbBytes[p] && !devRgb[p])) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_prepare_device: NULL tile bitmap, or NULL colour stream with a length");
        if (bitmapBytes[p] < need[p]) return yk_refuse(c, YK_ERR_RANGE, "yk_decode_prepare_device: tile bitmap shorter than the image needs");
        if (!yk_dpass_fits_key(need[p]) || rgbBytes[p] > 0xFFFFFFFFu)
            return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_prepare_device: a pass of 2^25 tile slots or more, or a colour stream of 4 GB or more; decode such an image window by window (yk_decode_set_window)");
    }
    const bool has1d = typeBytes != 0 || pixBytes != 0;
    if (has1d && (!devType || !devPix || compressionRange <= 0))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_prepare_device: 1-D streams need both pointers and a positive compressionRange (no 1-D chunk: both lengths 0)");
    YK_HIP(c, hipSetDevice(c->device));
    if (!c->dPrep) c->dPrep = new YkDecPrepared();
    YkDecPrepared& P = *c->dPrep;
    const YkDecView V = yk_dec_frame(c);
    // 1. the tile bitmaps and the 1-D streams into the handle's own buffer: the caller's may go once this call's work is done
    auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    size_t oBm[7] = {}, at = 0;
    for (int p = 0; p < nPasses; p++) { oBm[p] = at; at += up16(need[p]); }
    const size_t oTy = at, oPx = oTy + up16(typeBytes);
    at = oPx + up16(pixBytes);
    // every allocation first: a failure up to the first launch leaves the image as yk_decode_begin left it, and prepare may be called again
    const size_t T8 = (size_t)tilesW * (h >> 3), nb = (T8 + 1023) / 1024;
    const size_t oBT = 0, oBP = oBT + nb + 4, oTot = oBP + nb + 4, oOff = oTot + 16;          // in words
    const size_t nBlocks64 = (size_t)((w + 63) / 64) * ((h + 63) / 64);
    YK_HIP(c, P.streams.reserve(c->stream, at + 64));
    if (has1d) YK_HIP(c, P.d1.reserve(c->stream, oOff + T8 + 16));
    YK_HIP(c, P.table.reserve(c->stream, nBlocks64 + 2 * 1024));                // a render call's largest table: no allocation on the render path
    P.pl = DecPlan{};
    yk_dplan_shape(P.pl, nPasses, tileShiftX, tileShiftY, need);
    const DecAllScratch L = yk_decall_scratch(P.pl);
    if (nPasses) { const int rc = yk_dec_scratch(c, L.bytes); if (rc) return rc; }
    for (int p = 0; p < nPasses; p++) YK_HIP(c, hipMemcpyAsync(P.streams + oBm[p], devBitmap[p], need[p], hipMemcpyDeviceToDevice, c->stream));
    if (typeBytes) YK_HIP(c, hipMemcpyAsync(P.streams + oTy, devType, typeBytes, hipMemcpyDeviceToDevice, c->stream));
    if (pixBytes) YK_HIP(c, hipMemcpyAsync(P.streams + oPx, devPix, pixBytes, hipMemcpyDeviceToDevice, c->stream));
    for (int p = 0; p < nPasses; p++) { P.pl.bm[p] = P.streams + oBm[p]; P.pl.rgb[p] = devRgb[p]; P.pl.rgbBytes[p] = (uint32_t)rgbBytes[p]; }
    P.has1d = has1d; P.type = P.streams + oTy; P.typeBytes = typeBytes; P.pix = P.streams + oPx; P.pixBytes = pixBytes;
    P.invRange = has1d ? (1 << 24) / compressionRange : 0;
    if (has1d) { P.bT = P.d1 + oBT; P.bP = P.d1 + oBP; P.tot = P.d1 + oTot; P.offInBlk = P.d1 + oOff; }
    // from the first launch on the image's arrays are written: a HIP failure below leaves the image neither fresh nor prepared, and the chunk
    // calls, yk_decode_set_window and a second prepare refuse until the next yk_decode_begin
    c->dChunkSeen = true;
    if (nPasses) {
        // 2. the lattice: first touchers, count, scan, emit -- the launches of yk_decode_gradient_all_device; the corner colours are consumed here
        const DecPlan& pl = P.pl;
        const size_t nbTot = pl.blockStart[7], nBytesTot = pl.byteStart[7], lat = (size_t)latW * (h / 4 + 1);
        uint32_t* blockSums = reinterpret_cast<uint32_t*>(c->dScratch + L.oSums);
        uint32_t* perThread = reinterpret_cast<uint32_t*>(c->dScratch + L.oPerThread);
        YK_HIP(c, hipMemsetAsync(V.owner, 0xFF, lat * 4, c->stream));
        { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
        hipLaunchKernelGGL(yk_decall_owner_kernel, dim3((unsigned)((nBytesTot + 255) / 256)), dim3(256), 0, c->stream, pl, w, h, latW, V.loaded, V.owner);
        hipLaunchKernelGGL(yk_decall_stream_kernel<false>, dim3((unsigned)nbTot), dim3(1024), 0, c->stream, pl, w, h, latW, V.loaded, V.owner, blockSums, perThread,
                           (uint8_t*)nullptr, 0u);
        hipLaunchKernelGGL(yk_decall_scan_kernel, dim3(1), dim3(1024), 0, c->stream, blockSums, pl);
        hipLaunchKernelGGL(yk_decall_stream_kernel<true>, dim3((unsigned)nbTot), dim3(1024), 0, c->stream, pl, w, h, latW, V.loaded, V.owner, blockSums, perThread,
                           V.mapRGB, yk_dec_remap_factor(remapRange));
        // the emit launch above was the last reader of the corner colours (it took the plan by value): the kept plan forgets the caller's buffers
        for (int p = 0; p < nPasses; p++) { P.pl.rgb[p] = nullptr; P.pl.rgbBytes[p] = 0; }
        // 3. the marks of every block and no pixel: the window form with an empty rectangle
        hipLaunchKernelGGL(yk_decall_render_blocks_win_kernel, dim3((unsigned)(((w + 63) / 64) * ((h + 63) / 64))), dim3(256), 0, c->stream, pl, w, h, latW,
                           V.mapRGB, V.planes, c->dPlaneSize, w >> 3, reinterpret_cast<uint32_t*>(V.tile4), (w + 15) >> 4, DWinRect{ 0, 0, 0, 0 });
        YK_HIP(c, hipGetLastError());
        { int rc2 = yk_stage_end(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
    }
    if (has1d) {
        // 4. where every tile's parameters and pixels lie in the 1-D streams, from the whole mask
        { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_1D); if (rc2) return rc2; }
        hipLaunchKernelGGL(yk_dec1d_count_kernel, dim3((unsigned)nb), dim3(1024), 0, c->stream, V.tile4, (w + 15) >> 4, tilesW, T8, P.bT, P.bP, P.offInBlk);
        hipLaunchKernelGGL(yk_dec1d_scan_kernel, dim3(1), dim3(1024), 0, c->stream, P.bT, P.bP, (int)nb, P.tot);
        YK_HIP(c, hipGetLastError());
        { int rc2 = yk_stage_end(c, YK_STAGE_DEC_1D); if (rc2) return rc2; }
    }
    yk_wb_reset(P.blocks, w, h);
    // every rendered block gets its unmarked cells from the render call (the 1-D tiles, or zeros): nothing is left for yk_dec_settle, which
    // would write blocks no window asked for
    c->dPlanesStale = false;
    c->dPrepared = true;
    return YK_OK;
}

int yk_decode_prepared_blocks(yk_ctx* c, int* rendered, int* total) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c) || !c->dPrepared) return yk_refuse(c, YK_ERR_STATE, "yk_decode_prepared_blocks: yk_decode_prepare_device first");
    if (rendered) *rendered = c->dPrep->blocks.rendered;
    if (total) *total = yk_wb_total(c->dPrep->blocks);
    return YK_OK;
}

// The render half of yk_decode_render_windows[_scaled]_device, after every check: the 64x64 blocks the windows touch that no earlier call rendered
// (full size, the bitmap is shared by both calls), and the windows' origins in HBM behind the block list (*devXYOut)
static int yk_dec_render_new_blocks(yk_ctx* c, int nWindows, const int* xy, int ww, int wh, const int** devXYOut) {
    YkDecPrepared& P = *c->dPrep;
    YK_HIP(c, hipSetDevice(c->device));
    const int w = c->dw, h = c->dh, latW = w / 4 + 1, tilesW = w >> 3, tilesH = h >> 3, stride4 = (w + 15) >> 4;
    const YkDecView V = yk_dec_frame(c);
    // the table's buffer and its pinned slot before the bitmap changes: a refusal up to here leaves every block as it was
    const size_t maxList = (size_t)yk_wb_total(P.blocks), words = maxList + 2 * (size_t)nWindows;
    YK_HIP(c, P.table.reserve(c->stream, maxList + 2 * 1024));                  // prepare has reserved this: no allocation here
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, words * 4, &slot, &host); if (rc) return rc; }
    yk_wb_take(P.blocks, nWindows, xy, ww, wh, P.list);
    const size_t nList = P.list.size();
    uint32_t* tab = static_cast<uint32_t*>(host);
    for (size_t i = 0; i < nList; i++) tab[i] = P.list[i];
    for (int i = 0; i < 2 * nWindows; i++) tab[nList + i] = (uint32_t)xy[i];
    { const int rc = yk_dec_table_upload(c, slot, P.table, (nList + 2 * (size_t)nWindows) * 4); if (rc) return rc; }
    const uint32_t* devList = P.table;
    *devXYOut = reinterpret_cast<const int*>(P.table + nList);
    if (nList) {
        const uint32_t xB64 = (uint32_t)P.blocks.nbx, nTiles = (uint32_t)nList * 64u;
        { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
        hipLaunchKernelGGL(yk_decall_render_blocks_list_kernel, dim3((unsigned)nList), dim3(256), 0, c->stream, P.pl, w, h, latW, V.mapRGB, V.planes, c->dPlaneSize, tilesW,
                           reinterpret_cast<uint32_t*>(V.tile4), stride4, devList);
        if (!P.has1d)                                                           // no 1-D chunk: what no gradient tile covers reads as zero
            hipLaunchKernelGGL(yk_dec_zero_unmarked_list_kernel, dim3((nTiles + 255) / 256, 3), dim3(256), 0, c->stream, V.tile4, c->dTile4Size, stride4, tilesW, tilesH,
                               devList, xB64, nTiles, V.planes, c->dPlaneSize);
        YK_HIP(c, hipGetLastError());
        { int rc2 = yk_stage_end(c, YK_STAGE_DEC_GRADIENT); if (rc2) return rc2; }
        if (P.has1d) {
            const D1List ls = { devList, xB64, (uint32_t)tilesW, (uint32_t)tilesH };
            { int rc2 = yk_stage_begin(c, YK_STAGE_DEC_1D); if (rc2) return rc2; }
            hipLaunchKernelGGL(yk_dec1d_list_kernel, dim3((nTiles + 64 * YK_D1_TPL - 1) / (64 * YK_D1_TPL), 3), dim3(256), 0, c->stream, (const uint32_t*)P.offInBlk, (size_t)nTiles, ls,
                               (const uint32_t*)P.bT, (const uint32_t*)P.bP, (const uint32_t*)P.tot, P.type, P.typeBytes, P.pix, P.pixBytes, P.invRange, V.planes, c->dPlaneSize);
            YK_HIP(c, hipGetLastError());
            { int rc2 = yk_stage_end(c, YK_STAGE_DEC_1D); if (rc2) return rc2; }
        }
    }
    return YK_OK;
}

int yk_decode_render_windows_device(yk_ctx* c, int nWindows, const int* xy, int ww, int wh, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t windowBytes,
                                    int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c) || !c->dPrepared) return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_device: yk_decode_prepare_device first");
    YkDecPrepared& P = *c->dPrep;
    if (P.blocks.w != c->dw || P.blocks.h != c->dh)                             // the kept state describes the image the buffers hold, or nothing is launched
        return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_device: the prepared image is not the one this handle holds; yk_decode_begin and yk_decode_prepare_device again");
    if (nWindows < 1 || nWindows > 1024) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_device: nWindows must be 1..1024");
    if (!xy) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_device: the window table is NULL");
    if (!yk_wb_windows_ok(P.blocks, nWindows, xy, ww, wh))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_device: x0, y0, ww, wh must be multiples of 8 with ww, wh >= 8 and every window inside the image");
    if (!devOut) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_device: devOut is NULL");
    if (channels != 3 && channels != 4) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_device: channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255)) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_device: alpha must be -1 (the decoded plane) or 0..255");
    if (planeBytes == 0 ? rowBytes < (size_t)ww * channels : (rowBytes < (size_t)ww || planeBytes / (size_t)wh < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_device: row or plane pitch too small for the window");
    if (nWindows > 1 && (planeBytes == 0 ? windowBytes / (size_t)wh < rowBytes : windowBytes / (size_t)channels < planeBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_device: window stride too small for a window");
    const bool fromPlane = channels == 4 && alpha < 0;
    if (fromPlane && !c->dAlphaValid) return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_device: alpha = -1 needs yk_decode_alpha first");
    const int* devXY = nullptr;
    { const int rc = yk_dec_render_new_blocks(c, nWindows, xy, ww, wh, &devXY); if (rc) return rc; }
    const YkDecView V = yk_dec_frame(c);
    const int w = c->dw, tilesW = w >> 3;
    YkDetileArgs a;
    a.planes = V.planes; a.planeSize = c->dPlaneSize;
    a.alpha = fromPlane ? yk_dec_alpha_cur(c) : nullptr; a.strideA = (size_t)w; a.alphaConst = (uint32_t)((fromPlane ? 0 : alpha) & 255) * 0x01010101u;
    a.out = devOut; a.rowBytes = rowBytes; a.planeBytes = planeBytes;
    a.tileW = (uint32_t)tilesW; a.nTiles = (uint32_t)(ww >> 3) * (uint32_t)(wh >> 3);
    const uint32_t wtW = (uint32_t)(ww >> 3);
    const bool planar = planeBytes > 0;
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_DETILE); if (rc) return rc; }
    if (channels == 3) { if (planar) yk_dt_launch_wins<3, true, YK_DT_ALPHA_NONE>(a, c->stream, nWindows, devXY, wtW, windowBytes); else yk_dt_launch_wins<3, false, YK_DT_ALPHA_NONE>(a, c->stream, nWindows, devXY, wtW, windowBytes); }
    else if (fromPlane) { if (planar) yk_dt_launch_wins<4, true, YK_DT_ALPHA_PLANE>(a, c->stream, nWindows, devXY, wtW, windowBytes); else yk_dt_launch_wins<4, false, YK_DT_ALPHA_PLANE>(a, c->stream, nWindows, devXY, wtW, windowBytes); }
    else { if (planar) yk_dt_launch_wins<4, true, YK_DT_ALPHA_CONST>(a, c->stream, nWindows, devXY, wtW, windowBytes); else yk_dt_launch_wins<4, false, YK_DT_ALPHA_CONST>(a, c->stream, nWindows, devXY, wtW, windowBytes); }
    YK_HIP(c, hipGetLastError());
    return yk_stage_end(c, YK_STAGE_DEC_DETILE);
}

// yk_decode_render_windows_device for windows at any pixel offset and size: the blocks the pixel rectangles touch are rendered (the
// bitmap shared with the aligned and the scaled call), then every window's shared cover is de-tiled and clipped.  A cover may reach into a block
// no window touches: its bytes are loaded and clipped away, never written.
int yk_decode_render_windows_px_device(yk_ctx* c, int nWindows, const int* xy, int ww, int wh, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t windowBytes,
                                       int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!yk_dec_begun(c) || !c->dPrepared) return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_px_device: yk_decode_prepare_device first");
    YkDecPrepared& P = *c->dPrep;
    if (P.blocks.w != c->dw || P.blocks.h != c->dh)
        return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_px_device: the prepared image is not the one this handle holds; yk_decode_begin and yk_decode_prepare_device again");
    if (nWindows < 1 || nWindows > 1024) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_px_device: nWindows must be 1..1024");
    if (!xy) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_px_device: the window table is NULL");
    const int w = c->dw, h = c->dh;
    if (!yk_wpx_windows_ok(nWindows, xy, ww, wh, w, h))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_px_device: x0, y0 >= 0, ww, wh >= 1 and every window inside the image");
    if (!devOut) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_px_device: devOut is NULL");
    if (channels != 3 && channels != 4) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_px_device: channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255)) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_px_device: alpha must be -1 (the decoded plane) or 0..255");
    if (planeBytes == 0 ? rowBytes < (size_t)ww * channels : (rowBytes < (size_t)ww || planeBytes / (size_t)wh < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_px_device: row or plane pitch too small for the window");
    if (nWindows > 1 && (planeBytes == 0 ? windowBytes / (size_t)wh < rowBytes : windowBytes / (size_t)channels < planeBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_px_device: window stride too small for a window");
    const bool fromPlane = channels == 4 && alpha < 0;
    if (fromPlane && !c->dAlphaValid) return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_px_device: alpha = -1 needs yk_decode_alpha first");
    bool aligned = true;
    for (int k = 0; aligned && k < nWindows; k++) aligned = yk_wpx_aligned(xy[2 * k], xy[2 * k + 1], ww, wh);
    if (aligned) return yk_decode_render_windows_device(c, nWindows, xy, ww, wh, devOut, rowBytes, planeBytes, windowBytes, channels, alpha);
    const int* devXY = nullptr;
    { const int rc = yk_dec_render_new_blocks(c, nWindows, xy, ww, wh, &devXY); if (rc) return rc; }   // yk_wb_take works in pixels: any rectangle
    YkDetileArgs a;
    a.planes = yk_dec_frame(c).planes; a.planeSize = c->dPlaneSize;
    a.alpha = fromPlane ? yk_dec_alpha_cur(c) : nullptr; a.strideA = (size_t)w; a.alphaConst = (uint32_t)((fromPlane ? 0 : alpha) & 255) * 0x01010101u;
    a.out = devOut; a.rowBytes = rowBytes; a.planeBytes = planeBytes;
    a.tileW = (uint32_t)(w >> 3); a.nTiles = (uint32_t)(yk_wpx_shared_size(ww, w) >> 3) * (uint32_t)(yk_wpx_shared_size(wh, h) >> 3);
    const bool planar = planeBytes > 0;
    const unsigned gx = (a.nTiles + YK_DT_TILES - 1) / YK_DT_TILES;
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_DETILE); if (rc) return rc; }
    yk_dt_each(channels, planar, fromPlane, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((yk_dec_detile_wins_px_kernel<T::c, T::planar, T::asrc>), dim3(gx, (unsigned)nWindows), dim3(YK_DT_THREADS), 0, c->stream, a, devXY, ww, wh, w, h,
                           windowBytes);
    });
    YK_HIP(c, hipGetLastError());
    return yk_stage_end(c, YK_STAGE_DEC_DETILE);
}

// yk_decode_render_windows_device with reduced crops: the same render of new blocks (full size, the shared bitmap), then the scaled de-tile
int yk_decode_render_windows_scaled_device(yk_ctx* c, int level, int nWindows, const int* xy, int ww, int wh, uint8_t* devOut, size_t rowBytes, size_t planeBytes,
                                           size_t windowBytes, int channels, int alpha) {
    if (!c) return YK_ERR_BAD_ARG;
    if (level < 0 || level > 3) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: level must be 0..3");
    if (level == 0) return yk_decode_render_windows_device(c, nWindows, xy, ww, wh, devOut, rowBytes, planeBytes, windowBytes, channels, alpha);
    if (!yk_dec_begun(c) || !c->dPrepared) return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_scaled_device: yk_decode_prepare_device first");
    YkDecPrepared& P = *c->dPrep;
    if (P.blocks.w != c->dw || P.blocks.h != c->dh)
        return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_scaled_device: the prepared image is not the one this handle holds; yk_decode_begin and yk_decode_prepare_device again");
    if (nWindows < 1 || nWindows > 1024) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: nWindows must be 1..1024");
    if (!xy) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: the window table is NULL");
    if (!yk_wb_windows_ok(P.blocks, nWindows, xy, ww, wh))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: x0, y0, ww, wh (full-resolution pixels) must be multiples of 8 with ww, wh >= 8 and every window inside the image");
    if (!devOut) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: devOut is NULL");
    if (channels != 3 && channels != 4) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: channels must be 3 or 4");
    if (channels == 4 && (alpha < -1 || alpha > 255)) return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: alpha must be -1 (the decoded plane) or 0..255");
    const size_t rw = (size_t)ww >> level, rh = (size_t)wh >> level;
    if (planeBytes == 0 ? rowBytes < rw * channels : (rowBytes < rw || planeBytes / rh < rowBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: row or plane pitch too small for the reduced window");
    if (nWindows > 1 && (planeBytes == 0 ? windowBytes / rh < rowBytes : windowBytes / (size_t)channels < planeBytes))
        return yk_refuse(c, YK_ERR_BAD_ARG, "yk_decode_render_windows_scaled_device: window stride too small for a reduced window");
    const bool fromPlane = channels == 4 && alpha < 0;
    if (fromPlane && !c->dAlphaValid) return yk_refuse(c, YK_ERR_STATE, "yk_decode_render_windows_scaled_device: alpha = -1 needs yk_decode_alpha first");
    const int* devXY = nullptr;
    { const int rc = yk_dec_render_new_blocks(c, nWindows, xy, ww, wh, &devXY); if (rc) return rc; }
    YkDetileArgs a;
    a.planes = yk_dec_frame(c).planes; a.planeSize = c->dPlaneSize;
    a.alpha = fromPlane ? yk_dec_alpha_cur(c) : nullptr; a.strideA = (size_t)c->dw; a.alphaConst = (uint32_t)((fromPlane ? 0 : alpha) & 255) * 0x01010101u;
    a.out = devOut; a.rowBytes = rowBytes; a.planeBytes = planeBytes;
    a.tileW = (uint32_t)(c->dw >> 3); a.nTiles = (uint32_t)(ww >> 3) * (uint32_t)(wh >> 3);
    const YkDtsForm f = { 0, 0, 0, 0, nullptr, nWindows, devXY, (uint32_t)(ww >> 3), windowBytes };
    return yk_dts_run(c, a, f, level, channels);
}

}  // extern "C"
