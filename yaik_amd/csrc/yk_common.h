// Internal header shared by the HIP translation units of libyaik_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <memory>
#include <string>
#include <vector>
#include "../../include/yaik_hip.h"
#include "yk_udiv.h"

#define YK_BLK      64      // pixels per workgroup block side (= the 64x64 swizzle block of include/YAIK_private.h:212)
#define YK_LSTRIDE  68      // LDS row pitch in 32-bit words (65 used, 16-byte aligned rows)
#define YK_LROWS    65
#define YK_EV_RING  64
#define YK_SLOT     32      // bytes of nibble slot per 8x8 tile-plane (64 nibbles)
#define YK_NUM_STAGES 11    // YK_STAGE_* of include/yaik_hip.h
#define YK_STAGE_RING 16

// Batches: one handle can hold nFrames images of one shape; every per-image array is allocated nFrames times back to back and
// the batch kernels address frame f at base + f * stride (elements of the array's own type).
struct YkFrameStrides {
    unsigned long long plane, keep, bitmap[7], coverage, tileDef, tileCount, slots, blockN, defsOut, nibOut;   // bounds: 16 ints, totals: 8 u32
    unsigned long long bm0b, tileInfo, runSums;   // the fused kernel's per-strip 16x16 bytes (u8), per-tile records (8 bytes each), run sums (u32)
};

// The timing events of a handle: sets of {alpha begin, encode begin, encode end, pack end}, stand-alone records on the launch stream.  "encode
// begin" sits behind the ordering wait and is the end of the alpha interval as well, so ONE record separates the alpha kernel from the fused
// kernel; "encode end" is also the event another handle's fused kernel waits on (yk_order_fused_after).  Shared ownership: that handle holds
// on to the ring, so the event outlives this handle.
enum { YK_EVSET_ALPHA = 1, YK_EVSET_PACK = 2 };
enum { YK_EV_A0, YK_EV_E0, YK_EV_E1, YK_EV_P1, YK_EV_N };
struct YkEvRing {
    hipEvent_t ev[YK_EV_RING][YK_EV_N] = {};
    YkEvRing() = default;
    YkEvRing(const YkEvRing&) = delete; YkEvRing& operator=(const YkEvRing&) = delete;
    ~YkEvRing() { for (auto& set : ev) for (hipEvent_t e : set) if (e) (void)hipEventDestroy(e); }
};

// Device memory a handle owns: pointer and capacity in one place, one owner, freed with it.  `cap` counts elements of T (the bytes of padding
// some kernels read past the nominal end are asked for separately and are not part of it).  Two ways of getting memory, both on the handle's
// stream; either leaves the buffer EMPTY when it fails, never dangling and never with a stale capacity.  The caller reports the error
// (YK_HIP, or yk_refuse where a refusal leaves the handle usable).  Not copyable; movable, so that a group of buffers is released by
// assigning an empty group (c->img = YkImageBufs()).
template <class T> struct YkBuf {
    T* p = nullptr; size_t cap = 0;
    YkBuf() = default;
    YkBuf(const YkBuf&) = delete; YkBuf& operator=(const YkBuf&) = delete;
    YkBuf(YkBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    YkBuf& operator=(YkBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~YkBuf() { release(); }
    operator T*() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // exact: for the per-shape arrays that are re-made (and may shrink) when the shape or the frame count changes
    hipError_t alloc(hipStream_t s, size_t n, size_t padBytes = 0) {
        if (p) { const hipError_t e = hipStreamSynchronize(s); release(); if (e != hipSuccess) return e; }     // queued work may still use the old buffer
        const size_t bytes = n * sizeof(T) + padBytes;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes ? bytes : 16);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = n;
        return hipSuccess;
    }
    // grow-only: nothing happens while n elements fit
    hipError_t reserve(hipStream_t s, size_t n, size_t padBytes = 0) { return (p && cap >= n) ? hipSuccess : alloc(s, n, padBytes); }
};

struct YkEncodeParams {
    const int32_t* plane[4];
    int strideElems;
    int w, h;               // owned region (stripe): w = full width, h = owned rows
    int hAvail;             // rows physically present in the bound planes (h + halo)
    int y0;                 // first owned row in full-image coordinates
    int fullH;
    int rejectFactor, startMode, wantDst;
    int ablate;             // timing-only ablation switches (yk_set_ablation); 0 in every product run
    // alpha / bounds (device memory, written by the alpha kernels)
    const uint8_t* keep;    // per 16x16 macro-tile keep flag of this stripe, nullptr = no alpha plane
    const int32_t* bounds;  // [0..3] boundX0,Y0,X1,Y1 of the kept tiles (full-image pixels; yk_encode2_kernel derives the discard rule from them), [4] discardRejects for the first-generation kernel
    // outputs
    uint8_t* bitmap[7];
    uint16_t* coverage;     // per macro-tile, bit = cellY*4+cellX
    uint16_t* tileDef;      // [3][tilesW*tilesH]
    uint8_t*  tileCount;    // [3][tilesW*tilesH]
    uint8_t*  slots;        // [3][tilesW*tilesH][32]
    uint32_t* blockCnt;     // [ceil(tiles/1024)][2]: nibbles and coded tiles per scan block (atomics; nullptr = the scan counts itself)
    int32_t*  dst[3];
    int tilesW, tilesH, mtW, mtH;
    int xBB64, yBB64, xBB32, yBB32;
    int nFrames;            // 1 unless launched by yk_encode_batch
    const uint8_t* qtab;    // quantiser table of yk_encode2_kernel (yk_qtab_get)
    // yk_encode2_kernel's small outputs live in ONE allocation, so that lanes holding different outputs can share a store instruction (scalar base
    // + 32-bit lane offset): byte offsets, inside `small`, of frame 0 of the seven bitmaps (= bitmap[i]), of the strips' 16x16 bytes (4 bits each:
    // yk_scan2_kernel folds them into bitmap[0]), the coverage words (= coverage), the per-tile records {def0 | def1 << 16, def2 | count << 16}
    // and the per-run sums {nibbles / 16 | coded tiles << 16} (one per 8 consecutive tiles; widths that are multiples of 8 tiles only)
    uint8_t* small;
    uint32_t oBm[7], oBm0b, oCov, oInfo, oRun;
    // optional (yk_set_pixel_cache): the packed pixels (0x00BBGGRR) of every 4x4 cell the gradient passes left uncovered, for the live 1-D range
    // path behind the fused kernel, which then reads 4 bytes per such pixel instead of 12 from the planes: [strip (row-major)][cell row 0..3][lane]
    // 16-byte pieces, lane in this kernel's (Morton) order.  nullptr = not wanted.
    uint4* pixCache;
    YkFrameStrides fs;
    // yk_encode2_kernel's unit decode: block -> frame and block -> block row without the runtime's integer division (yk_udiv.h; computed when
    // the image or batch is set).  A launch keeps every block index below YK_UDIV_LIMIT (yk_launch_encode2).
    YkUdiv divXBB64, divNBf;
    // yk_encode2_kernel's per-strip bitmap words and run sums: where lane k of a strip stores, as a table built once per handle
    // (yk_out_table_fill) instead of ~200 scalar instructions per strip.  The rows hold offsets of frame 0; outFrame0 is the frame a
    // single-frame launch works on (its oBm.. above are already moved on to that frame).
    const uint4* outTab;
    uint32_t outFrame0;
};

// ---- yk_encode2_kernel's output table.  A strip (block BX, BY, strip `wave` of the block, frame fr) stores its share of the seven swizzled
// bitmaps and its two run sums at offsets into the small-output arena that are all affine in (fr, BX, BY) once `wave` is fixed.  Row
// [wave][k] describes what lane k < 16 of such a strip stores:
//   offset = base + fr * sF + BX * sX + BY * sY   if BX < limX and BY < limY, else nothing (the bitmaps of 32-pixel blocks and the run sums end
//            inside a 64x64 block at the right and bottom edges; a row nothing is stored from has limX = 0)
//   value  = (s_bm[sel & 31] >> ((sel >> 8) & 31)) & (~0u >> (sel >> 16))     (rows 11, 12: the run sums, computed by the strip)
// lanes 1..3 store bytes, 4..6 16-bit words, 8..12 32-bit words: one store per access width, every lane with at most one output.
#define YK2_OT_ROWS 16
#define YK2_OT_NONE 0xFFFFFFFFu
struct YkOutRow { uint32_t base, sF, sX, sY, limX, limY, sel, pad; };
static_assert(sizeof(YkOutRow) == 32, "two 16-byte loads per row");
struct YkOutGeom { uint32_t oBm[7], oBm0b, oRun; int xBB64, xBB32, yBB32, tilesW, tilesH; };   // offsets of frame 0 inside the arena
inline void yk_out_table_fill(YkOutRow (*T)[YK2_OT_ROWS], const YkOutGeom& g, const YkFrameStrides& fs) {
    const uint32_t none = YK2_OT_NONE;
    auto lim = [](int n, int step) -> uint32_t { return n <= 0 ? 0u : (uint32_t)((n + step - 1) / step); };   // count of B >= 0 with B * step < n
    for (int wv = 0; wv < 4; wv++) {
        const uint32_t w1 = (uint32_t)wv & 1u, w2 = (uint32_t)wv >> 1, X64 = (uint32_t)g.xBB64, X32 = (uint32_t)g.xBB32;
        YkOutRow* R = T[wv];
        for (int k = 0; k < YK2_OT_ROWS; k++) R[k] = YkOutRow{ 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
        auto sel = [](uint32_t idx, uint32_t sh, uint32_t bits) { return idx | (sh << 8) | ((32u - bits) << 16); };
        // bytes: 16x16 (4 bits of the strip), 16x8, 8x16 -- byte `wave` of the block's word
        R[1] = YkOutRow{ g.oBm0b + wv, (uint32_t)fs.bm0b, 4u, 4u * X64, none, none, sel(0, 4u * wv, 4), 0u };
        R[2] = YkOutRow{ g.oBm[1] + wv, (uint32_t)fs.bitmap[1], 4u, 4u * X64, none, none, sel(1, 8u * wv, 32), 0u };
        R[3] = YkOutRow{ g.oBm[2] + wv, (uint32_t)fs.bitmap[2], 4u, 4u * X64, none, none, sel(2, 8u * wv, 32), 0u };
        // 16-bit words: 8x8, then 4x8 in the two 32x64 swizzle blocks of the 64x64 block
        R[4] = YkOutRow{ g.oBm[3] + 2u * wv, (uint32_t)fs.bitmap[3], 8u, 8u * X64, none, none, sel(3 + w2, 16u * w1, 32), 0u };
        for (uint32_t sx = 0; sx < 2; sx++)
            R[5 + sx] = YkOutRow{ g.oBm[5] + (sx * 4u + wv) * 2u, (uint32_t)fs.bitmap[5], 16u, 8u * X32, lim(g.xBB32 - (int)sx, 2), none, sel(9 + sx * 2 + w2, 16u * w1, 32), 0u };
        // 32-bit words: 8x4 (64x32 swizzle blocks), 4x4 (32x32 swizzle blocks), the sums of the strip's two runs of eight tiles
        const uint32_t limY32 = lim(g.yBB32 - (int)w2, 2);
        R[8] = YkOutRow{ g.oBm[4] + w2 * 8u * X64 + w1 * 4u, (uint32_t)fs.bitmap[4], 8u, 16u * X64, none, limY32, sel(5 + w2 * 2 + w1, 0, 32), 0u };
        for (uint32_t sx = 0; sx < 2; sx++)
            R[9 + sx] = YkOutRow{ g.oBm[6] + w2 * 8u * X32 + sx * 8u + w1 * 4u, (uint32_t)fs.bitmap[6], 16u, 16u * X32, lim(g.xBB32 - (int)sx, 2), limY32,
                                  sel(13 + (w2 * 2 + sx) * 2 + w1, 0, 32), 0u };
        if ((g.tilesW & 7) == 0) {                              // other widths add to the scan block's counters instead
            const uint32_t runsW = (uint32_t)(g.tilesW >> 3);
            for (int r = 0; r < 2; r++)
                R[11 + r] = YkOutRow{ g.oRun + (uint32_t)(wv * 2 + r) * runsW * 4u, (uint32_t)fs.runSums * 4u, 4u, 32u * runsW, none, lim(g.tilesH - wv * 2 - r, 8), 0u, 0u };
        }
    }
}

// yk_encode_streams_batch (yk_streams_batch.hip): one record per frame in HBM, the bases of the frame's streams in the batch's output buffer
// (nullptr: empty or not requested); the emit kernels read the record of their frame through uniform loads
#define YK_SB_COUNTS 9          // uint32 read back per frame: corners of the 7 passes, coded 1-D tiles and 1-D pixel bytes of one plane
struct YkStreamRec { uint8_t* rgb[7]; uint8_t* pix; uint8_t* type; };
// the batch's own buffers (grow-only, freed with the image): they share nothing with the single-image corner / 1-D state
struct YkStreamsBatch {
    YkBuf<uint32_t> owner;                                       // [F][lattice]
    YkBuf<uint32_t> cScratch;                                    // [F][block sums], [F][ownership words]
    YkBuf<uint32_t> r1Scratch;                                   // [F][offsets in block], [F][coded tiles per block], [F][pixel bytes per block]
    YkBuf<uint32_t> counts;                                      // [F][YK_SB_COUNTS]
    YkBuf<uint8_t> out;                                          // every stream of every frame, each on a multiple of 16
    YkBuf<YkStreamRec> tab;                                      // [F]
    std::vector<yk_frame_streams> table; bool valid = false;     // what yk_batch_streams_table hands out
    int what = 0;                                                // the YK_STREAMS_* the valid table was built with
};

// yk_palette_compress* (yk_palette.hip): PaletteCompressor over a list of segments.  Everything is grow-only and belongs to the handle.
struct YkPalette {
    YkBuf<uint8_t> scratch;                                      // segment table, vote tables, candidates, books, tokens, offsets, lengths
    YkBuf<uint8_t> out;                                          // the payloads of the last call, each on a multiple of 16
    YkBuf<uint32_t> carry;                                       // the 64 find-table rows that carry from call to call (packed deltas)
    bool carryFresh = true;                                      // the carried rows are those of a fresh process (all zero deltas)
    std::vector<uint8_t> segHost;                                // the segment table on its way to HBM
    std::vector<uint32_t> lenBase;                               // read back: [nSeg] payload lengths, [nSeg] payload offsets in `out`
    int nSeg = 0; bool valid = false;
};

// yk_palette_decompress_streams (yk_palette_dec.hip): PaletteDecompressor over a list of payloads.  Grow-only, owned by the handle.
struct YkPaletteDec {
    YkBuf<uint8_t> scratch;                                      // stream table, chunk records, token offsets, colour records, halos, status words
    YkBuf<uint8_t> out;                                          // the decoded streams of the last call, each on a multiple of 16, 64 free bytes around them
    YkBuf<uint8_t> stage;                                        // yk_decode_gradient_palette: the host's tile bitmap and payload on their way in
    std::vector<size_t> slotOff, slotLen;                        // where every stream's output lies in `out`
    std::vector<uint32_t> statusHost;
    size_t statusOff = 0;                                        // the status words inside `scratch`
    int nSeg = 0; bool valid = false;
};

// yk_alpha_kernel's work unit: YK_ALPHA_R rows of 16x16 tiles of one 256-pixel segment (one wave).  Every unit intersects the image.
#ifndef YK_ALPHA_R
#define YK_ALPHA_R 4
#endif
static inline size_t yk_alpha_units(int fullW, int mtH) { return (size_t)((fullW / 4 + 63) / 64) * (size_t)((mtH + YK_ALPHA_R - 1) / YK_ALPHA_R); }

// Everything that is allocated for one image shape and frame count (yk_set_image, yk_set_batch) or grows with the work done on it, and goes
// when the shape changes: released as a whole (yk_free_image).  The pointers the kernels are given -- the frame-0 bases B, the per-frame
// views of yk_frame, the pieces of `small` -- point into these.
struct YkImageBufs {
    // alpha
    YkBuf<uint8_t> keep; YkBuf<int32_t> bounds;
    YkBuf<int> alphaUnitBox;            // yk_alpha_kernel: one box {x0, y0, x1, y1} per work unit (yk_alpha_units) and frame, folded by yk_alpha_box_kernel
    // encode outputs and compaction
    YkBuf<uint8_t> small;               // one allocation: bitmap[0..6], bm0b, coverage, tileInfo, runSums (each nFrames times)
    YkBuf<uint4> outTab;                // yk_encode2_kernel's output table (yk_out_table_fill): [4 strips of a block][YK2_OT_ROWS] rows of 32 bytes
    YkBuf<uint16_t> tileDef; YkBuf<uint8_t> tileCount, slots;
    YkBuf<int32_t> dst[3];
    YkBuf<uint32_t> blockSums, blockCnt, totals;
    YkBuf<unsigned long long> exportSizes;   // [16] total + section sizes of the last yk_export_tile_maps
    YkBuf<uint16_t> defsOut; YkBuf<uint8_t> nibOut;
    // corner streams
    YkBuf<uint32_t> latticeOwner; YkBuf<uint8_t> cornerStream; YkBuf<uint32_t> cornerScratch;
    YkBuf<uint32_t> cornerEdgeIdx;      // [2][w/4+1]: emission index (in corners, within its pass) of the first / last lattice row
    // plane-subset passes
    YkBuf<uint16_t> covCh;              // [3][covChStride]
    YkBuf<uint8_t> mapped3;             // bit p = plane p's corner at this lattice point has been emitted
    YkBuf<uint32_t> ppBitmap; YkBuf<uint8_t> ppStream; YkBuf<uint32_t> ppScratch;
    YkBuf<int32_t> preview;             // FittingQuadSmooth's testOutput planes (3 x w*h int32), INT32_MIN where no tile wrote
    // live 1-D range path and the pixel cache that feeds it
    YkBuf<uint8_t> r1Slots, r1Params; YkBuf<uint32_t> r1Cnt; YkBuf<uint8_t> r1Pix, r1Type;
    YkBuf<uint4> pixCache;              // yk_set_pixel_cache: uncovered cells' packed pixels, fused kernel -> 1-D path
    YkStreamsBatch sb;                  // yk_encode_streams_batch
};

// The layout of yk_ctx must NOT depend on YK_TEST_HOOKS: the product library and the test-hooks build of the same sources are loaded side by
// side by the tests, each owning the handles it created (yaik_amd/encoder.py keeps a handle with its library); no member below is conditional.
struct yk_ctx {
    int device = -1;
    int numCU = 256;             // compute units of the device (persistent grids are sized from it)
    const uint8_t* qtab = nullptr;   // per-device quantiser table (owned by the library, shared by all handles)
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    // geometry
    int fullW = 0, fullH = 0, nPlanes = 0, y0 = 0, h = 0, halo = 0;
    int tilesW = 0, tilesH = 0, mtW = 0, mtH = 0;
    // batch: B holds the address of every per-frame array for frame 0 and fs the per-frame strides, the one record of where things are;
    // yk_frame(c, f) computes the arrays of frame f from them, and the single-image entry points work on frame `curFrame`
    int nFrames = 1, curFrame = 0;
    YkFrameStrides fs = {};
    YkUdiv divXBB64 = {}, divNBf = {};   // yk_encode2_kernel's unit decode (yk_udiv.h), set with the image
    struct Bases {
        const int32_t* plane[4];        // the bound input planes (nullptr: not bound)
        uint8_t* keep;                  // mtW*mtH keep flags of the alpha stage
        int32_t* bounds;                // 16 ints: [0..4] the host-combined box of a striped image + its discard flag (yk_alpha_finish), [8..11] the box yk_alpha_box_kernel folds from the units of yk_alpha_kernel
        uint8_t* bitmap[7]; uint16_t* coverage; uint16_t* tileDef; uint8_t* tileCount; uint8_t* slots;   // encode outputs
        uint32_t* blockSums;            // [nBlocks][2]: exclusive prefix of (nibbles, coded tiles) per block of 1024 tiles, same for the 3 planes
        uint32_t* blockCnt;             // [nBlocks][2]: the sums themselves, accumulated by the fused kernel, consumed (and cleared) by the scan
        uint32_t* totals;               // [3][2]
        uint16_t* defsOut;              // [3][T8]
        uint8_t* nibOut;                // [3][T8*32 + 8]
        uint8_t* small;                 // one allocation: bitmap[0..6], bm0b, coverage, tileInfo, runSums (each nFrames times; the pointers above point into it)
        uint8_t* bm0b; uint2* tileInfo; uint32_t* runSums;
    } B = {};
    // input (the bound planes are B.plane)
    int strideElems = 0;
    YkBuf<int32_t> ownedPlanes;
    YkBuf<uint8_t> pxStage;                                 // yk_upload_pixels_u8: grow-only HBM copy of the host's 8-bit rows (16-byte pitch)
    hipEvent_t evPixCopy = nullptr;                         // ... recorded behind that copy: the call returns once the host rows are read
    // alpha
    int boundsOff = 8;                  // where the image-wide box is: 8 (whole image, batch) or 0 (stripes, after yk_alpha_finish)
    bool alphaDone = false, alphaFinished = false;
    int32_t hostBounds[4] = {0, 0, 0, 0}; int hostDiscard = 1, hostHasChunk = 0;
    // encode outputs
    size_t bitmapBytes[7] = {};
    int32_t dstFill = -1; bool dstValid = false;
    // compaction
    hipEvent_t evHandoff = nullptr;              // yk_stream_handoff / yk_stream_wait_for
    // yk_order_fused_after: the next fused kernel waits for this event, the end of the other handle's fused kernel.  It belongs to that handle's
    // ring, which fusedAfterRing keeps alive should the other handle be destroyed before this one encodes.
    hipEvent_t fusedAfter = nullptr; std::shared_ptr<YkEvRing> fusedAfterRing;
    size_t nibStride = 0;
    int nScanBlocks = 0;
    bool encoded = false;
    // corner streams
    bool cornersReady = false; int nextCornerPass = 0;
    size_t cornerOff[7] = {}, cornerBytes[7] = {};
    const uint32_t* cornerTotalsDev = nullptr; bool cornerTotalsPending = false;   // stream lengths still on the device (yk_corners_finish)
    const uint32_t* r1TotalsDev = nullptr; bool r1TotalsPending = false;           // the same for the 1-D path (yk_range1d_finish)
    // partial-plane gradient passes (FittingQuadSmooth with nullable planes): per-plane coverage (mapSmoothTile[p], u16 per 16x16 tile, bit = cell)
    // and per-plane "corner already emitted" flags per lattice point (mappedRGB[p]); allocated by the first partial pass after an encode (img)
    size_t covChStride = 0;
    size_t ppBitmapBytes = 0, ppStreamBytes = 0;               // bytes of the last plane-subset pass's bitmap and corner stream
    int ppAccepted = 0; bool ppActive = false;
    int ppLastBit = 0, ppLastSx = 0, ppLastSy = 0;         // the last plane-subset pass (its bitmap is img.ppBitmap)
    bool previewFresh = false;                             // img.preview holds INT32_MIN wherever no tile has written since the encode
    // (f)4 3-D LUT tiles (yk_lut3d.hip): pattern bank + the streams StartCorrelationSearch allocates
    struct YkLutState* lut = nullptr;
    struct YkLutDecState* lutDec = nullptr;      // decoder: the per-orientation tables YAIK_AssignLUT lays out
    // live 1-D range path (a15)
    uint32_t r1Tiles = 0, r1PixCount = 0; bool r1Ready = false;
    bool pixCacheOn = false, pixCacheValid = false;      // yk_set_pixel_cache (img.pixCache)
    uint32_t r1EndTiles[3] = {}, r1EndPix[3] = {};       // cumulative per plane (equal thirds unless a partial-plane pass ran)
    // decode
    int dw = 0, dh = 0; size_t dPlaneSize = 0, dTile4Size = 0;
    YkBuf<uint8_t> dScratch;
    bool dSplit = false;
    YkBuf<uint8_t> dAlpha; bool dAlphaValid = false;     // yk_decode_alpha: the w x h alpha plane of the image being decoded
    YkBuf<uint8_t> dAvScratch;                           // its payload, mask and row counts
    // yk_alpha_values[_batch], one layout: avState holds 8 ints per frame (box + class flags), avPay the frames' payload slots back to back
    // (each on a multiple of 16), avTab the records of the frames that have a box, in HBM
    YkBuf<int32_t> avState; YkBuf<uint8_t> avPay, avTab;
    // the 6-bit mask mode: tile prefixes, band scan, packed payload (yk_alpha_values); the record table, selected counts, prefix arena and 6-bit
    // slots of every such frame (yk_alpha_values_mask_batch)
    YkBuf<uint8_t> av6;
    // avBatch = what the payload getters hand out after yk_alpha_values[_mask]_batch (valid while avBatchValid; yk_alpha_values publishes no slot):
    // off is into avPay, for mode 3 into av6
    struct AvSlot { int32_t mode; size_t off, bytes; };
    std::vector<AvSlot> avBatch; bool avBatchValid = false;
    // yk_alpha_bitmaps_batch: the 'MIPM' bits of every frame, one slot of mipSlot bytes each (written whole by the kernel); mipBytes = the lengths
    // yk_alpha_bitmap_device hands out (valid while mipValid)
    YkBuf<uint8_t> mipBits; size_t mipSlot = 0; std::vector<uint32_t> mipBytes; bool mipValid = false;
    YkBuf<uint8_t> gatherTab;                            // yk_device_gather: piece prefixes and segment records in HBM
    // yk_decode_alpha_batch_device: dAlpha holds dFrames planes dAlphaStride bytes apart (the selected frame's is yk_dec_alpha_cur)
    bool dAlphaBatch = false; size_t dAlphaStride = 0;
    // yk_decode_alpha_mask_batch_device: the frames of modes 2 / 3 of the last batch call, in table order, and one status word for each of them
    std::vector<int32_t> dAvMaskFrames; YkBuf<int32_t> dAvStatus;
    // yk_decode_set_window: the rectangle (pixels, multiples of 8) the decode of this image has to produce; dWinSet false = the whole image.
    // dBatchBegun: the handle was begun by yk_decode_begin_batch (no windows there); dChunkSeen: a chunk of the image has been decoded
    int dWinX = 0, dWinY = 0, dWinW = 0, dWinH = 0;
    bool dWinSet = false, dBatchBegun = false, dChunkSeen = false;
    // yk_decode_set_batch_windows: one window per frame of the batch, all of dBWinW x dBWinH pixels.  dBWinTab holds frame f's exact rectangle
    // {x0, y0, x1, y1} (pixels) in HBM for the batch x window kernels: 1024 entries, allocated once, written through the pinned ring below
    bool dBWinSet = false; int dBWinW = 0, dBWinH = 0;
    YkBuf<int> dBWinTab;
    // yk_decode_set_window_px / yk_decode_set_batch_windows_px: the window above is the 8-aligned cover the chunk calls decode, and this
    // is the pixel rectangle the output call writes: dPx{X,Y} the single image's origin, dPx{W,H} the size (of every frame's window in a batch, whose
    // per-frame offsets into the cover lie in dBWinTab behind the rectangles, at int 4 * dFrames)
    bool dPxSet = false; int dPxX = 0, dPxY = 0, dPxW = 0, dPxH = 0;
    // yk_decode_output_norm_batch_device: the per-frame mirror flags in HBM: 1024 entries, allocated once, written through the pinned ring
    YkBuf<uint32_t> dNormTab;
    // yk_decode_set_batch_rects: a source rectangle per frame, each with its own 8-aligned cover.  The covers lie in dBWinTab like windows
    // and dBWinSet is set with them, so every call that refuses under windows refuses here; dBWinW x dBWinH is then the bounding size of the covers and
    // dBRectMaxTiles the largest cover's tile count (what the grids of the per-frame launches are sized by).  dBRects keeps the exact rectangles
    // {x0, y0, sw, sh} on the host for yk_decode_output_resampled_batch_device, whose nine words per frame go into dRsTab (1024 frames, allocated once)
    bool dBRectSet = false; uint32_t dBRectMaxTiles = 0;
    std::vector<int> dBRects;
    YkBuf<int> dRsTab;
    bool dPlanesStale = false;          // the planes were not cleared for this image: cells tile4x4Mask does not mark hold the previous image (yk_dec_settle)
    // yk_decode_prepare_device: the map-sized work of this image is done and what a render needs is kept in dPrep (yk_decode.hip) until the next
    // yk_decode_begin[_batch]; the buffers in dPrep are grow-only and go with the handle (yk_dec_prepared_free)
    bool dPrepared = false;
    struct YkDecPrepared* dPrep = nullptr;
    // decode batch (yk_decode_begin_batch): dB holds the allocations (frame 0) and dStride the distance in BYTES from one frame's array to the
    // next, like B / fs on the encode side; yk_dec_frame(c, f) computes the arrays of frame f, and the single-image entry points work on frame
    // `dCur`.  loaded: lattice point already popped from a colour stream (mapRGBMask)
    int dFrames = 1, dCur = 0;
    struct DBases { uint8_t* planes; uint8_t* mapRGB; uint32_t* owner; uint8_t* loaded; uint8_t* tile4; } dB = {};
    struct DFrames { YkBuf<uint8_t> planes, mapRGB; YkBuf<uint32_t> owner; YkBuf<uint8_t> loaded, tile4; } dFrm;   // what dB points into
    struct DStrides { size_t planes, mapRGB, owner, loaded, tile4; } dStride = {};
    // the per-frame tables of the batch calls on their way to HBM: a ring of pinned host buffers, each with the event behind its copy
    void* dTabHost[4] = {}; size_t dTabHostBytes[4] = {}; hipEvent_t dTabEv[4] = {}; unsigned dTabSeq = 0;
    // yk_decode_compare_*: the folded u64 results of every frame, then one record per workgroup (grow-only; yk_quality.hip)
    YkBuf<uint8_t> qBuf;
    // timing
    // timing events: a ring of YK_EV_RING sets (YkEvRing) so that a caller can run many frames back to back and read the per-kernel
    // averages afterwards without synchronising every frame
    std::shared_ptr<YkEvRing> evRing;
    unsigned evHead = 0, evTail = 0;      // sets [evTail, evHead) hold a completed encode; evCur = evHead % YK_EV_RING is being filled
    bool evAlphaInCur = false;
    uint8_t evHas[YK_EV_RING] = {};       // per set: YK_EVSET_ALPHA, YK_EVSET_PACK = these intervals were taken (the encode interval always is)
    float msEncode = 0, msAlpha = 0, msPack = 0;
    // stage timers (yk_stage_ms): HIP events around the kernel sections of the stages outside the fused encode, on the launch stream
    hipEvent_t stEv[YK_NUM_STAGES][YK_STAGE_RING][2] = {};
    int stN[YK_NUM_STAGES] = {};                 // event pairs recorded since the last fold
    double stAcc[YK_NUM_STAGES] = {}; int stCalls[YK_NUM_STAGES] = {};
    int ablate = 0;
    // whole-frame graph (yk_encode_frame): the stream operations of alpha stage + fused kernel + compaction, captured once per
    // (planes, shape, arguments) and replayed with one launch — for batches of small frames, where launches dominate
    hipGraphExec_t frameGraph = nullptr;
    unsigned long long frameGraphKey[12] = {};
    int kernelVersion = 2;              // 2 = yk_encode2_kernel; 1 = the registered cross-check launcher (tests/csrc/yk_encode_v1.hip)
    YkImageBufs img;                    // the per-image buffers, yk_encode_streams_batch's among them
    YkPalette pal;                      // yk_palette_compress*
    YkPaletteDec pdec;                  // yk_palette_decompress_streams, yk_decode_gradient_palette
};

// The arrays of ONE frame of the handle: yk_ctx::Bases moved on by the frame's strides.  These two functions are the only place where a frame
// index meets a stride; everything that works on one frame takes a view at its top and reads from it.
typedef yk_ctx::Bases YkFrameView;
inline YkFrameView yk_frame(const yk_ctx* c, int f) {
    const YkFrameStrides& fs = c->fs; const size_t n = (size_t)f;
    YkFrameView V = c->B;
    for (int i = 0; i < 4; i++) if (V.plane[i]) V.plane[i] += n * fs.plane;
    V.keep += n * fs.keep; V.bounds += n * 16; V.totals += n * 8;
    for (int i = 0; i < 7; i++) V.bitmap[i] += n * fs.bitmap[i];
    V.coverage += n * fs.coverage; V.tileDef += n * fs.tileDef; V.tileCount += n * fs.tileCount; V.slots += n * fs.slots;
    V.blockSums += n * fs.blockN; V.blockCnt += n * fs.blockN; V.defsOut += n * fs.defsOut; V.nibOut += n * fs.nibOut;
    V.bm0b += n * fs.bm0b; V.tileInfo += n * fs.tileInfo; V.runSums += n * fs.runSums;
    return V;                                                            // V.small stays the allocation: offsets into it are taken from there
}
inline YkFrameView yk_frame(const yk_ctx* c) { return yk_frame(c, c->curFrame); }
typedef yk_ctx::DBases YkDecView;
inline YkDecView yk_dec_frame(const yk_ctx* c, int f) {
    const yk_ctx::DStrides& s = c->dStride; const size_t n = (size_t)f;
    YkDecView V = c->dB;
    V.planes += n * s.planes; V.mapRGB += n * s.mapRGB; V.owner += n * s.owner / 4; V.loaded += n * s.loaded; V.tile4 += n * s.tile4;   // owner: the stride is bytes, a multiple of 16
    return V;
}
inline YkDecView yk_dec_frame(const yk_ctx* c) { return yk_dec_frame(c, c->dCur); }
// what the entry points ask before they work: an image is set (yk_set_image has allocated), planes are bound (a batch of more than one frame
// also needs its frame stride: yk_bind_device_batch), a decode has begun
inline bool yk_image_set(const yk_ctx* c) { return c->B.tileCount != nullptr; }
inline bool yk_planes_bound(const yk_ctx* c) { return c->B.plane[0] != nullptr; }
inline bool yk_batch_planes_bound(const yk_ctx* c) { return c->B.plane[0] && (c->nFrames == 1 || c->fs.plane != 0); }
inline bool yk_dec_begun(const yk_ctx* c) { return c->dB.planes != nullptr; }

int yk_fail(yk_ctx* c, int code, const char* what, hipError_t e = hipSuccess);
// yk_fail keeps the FIRST message of a handle (its callers rely on that); yk_refuse is for entry points whose refusals leave the handle usable and are
// met again and again (the decode batch calls): the message is always that of the latest refusal
int yk_refuse(yk_ctx* c, int code, const char* what);
#define YK_HIP(c, call) do { hipError_t _e = (call); if (_e != hipSuccess) return yk_fail((c), YK_ERR_HIP, #call, _e); } while (0)

// 'ALPM', 'MIPM', '3DTL' and plane-subset chunks act on one image: with a decode batch of more than one frame they refuse, touching nothing
#define YK_DEC_NO_BATCH(c, name) do { if ((c)->dFrames > 1) return yk_refuse((c), YK_ERR_STATE, name " is not supported in a batch (yk_decode_begin_batch with nFrames > 1)"); } while (0)

// the calls that hand out or compare the whole image refuse while a window is set: outside it the planes hold whatever they held before
// ... and while the image is prepared for windows (yk_decode_prepare_device): only the blocks some window asked for are rendered
// ... and while the frames of a batch have windows (yk_decode_set_batch_windows): the same holds per frame
#define YK_DEC_NO_BATCH_WINDOWS(c, name) do { \
    if ((c)->dBRectSet) return yk_refuse((c), YK_ERR_STATE, name " needs whole frames, but rectangles are set on this batch (yk_decode_set_batch_rects): use yk_decode_output_resampled_batch_device"); \
    if ((c)->dBWinSet) return yk_refuse((c), YK_ERR_STATE, name " needs whole frames, but windows are set on this batch (yk_decode_set_batch_windows): use yk_decode_output_batch_windows_device"); } while (0)
#define YK_DEC_NO_WINDOW(c, name) do { \
    YK_DEC_NO_BATCH_WINDOWS(c, name); \
    if ((c)->dWinSet) return yk_refuse((c), YK_ERR_STATE, name " needs the whole image, but a window is set on this decode (yk_decode_set_window): use yk_decode_output_window_device"); \
    if ((c)->dPrepared) return yk_refuse((c), YK_ERR_STATE, name " needs the whole image, but this image is prepared for windows (yk_decode_prepare_device): use yk_decode_render_windows_device"); } while (0)
// the chunk calls and the single-window calls: a prepared image takes no further chunk and hands out pixels through yk_decode_render_windows_device
#define YK_DEC_NO_PREPARED(c, name) do { if ((c)->dPrepared) return yk_refuse((c), YK_ERR_STATE, name ": this image is prepared for windows (yk_decode_prepare_device); yk_decode_render_windows_device reads it, yk_decode_begin starts the next image"); } while (0)

// launchers implemented in the kernel TUs
int yk_stage_begin(yk_ctx* c, int stage);                // records the begin event of a new interval of `stage` on c->stream
int yk_stage_end(yk_ctx* c, int stage);
int yk_launch_alpha(yk_ctx* c, bool batch = false);
int yk_launch_alpha_finish(yk_ctx* c, const int32_t* globalBBox);
int yk_launch_encode(yk_ctx* c, int rejectFactor, int mode3BitOnly, int wantDst, bool batch = false);
int yk_launch_pack(yk_ctx* c, bool batch = false);
int yk_launch_corners(yk_ctx* c);
int yk_launch_unpack_u8(yk_ctx* c, const uint8_t* src, size_t rowBytes, size_t frameBytes, int channels, int rows, int nFrames,
                        int32_t* dst, size_t planeElems, size_t frameElems);   // yk_pixels.hip
// yk_encode_streams_batch: count and emit phases over all frames (yk_corners.hip, yk_range1d.hip)
int yk_corners_batch_count(yk_ctx* c);
int yk_corners_batch_emit(yk_ctx* c);
int yk_range1d_batch_count(yk_ctx* c);
int yk_range1d_batch_emit(yk_ctx* c);
int yk_corners_finish(yk_ctx* c);                         // reads the corner streams' lengths back if that is still pending (synchronises)
// the pinned ring behind the per-frame tables of the decode batch calls (yk_decode.hip)
extern "C" int yk_dec_table_host(yk_ctx* c, size_t bytes, int* slot, void** host);
extern "C" int yk_dec_table_upload(yk_ctx* c, int slot, void* dev, size_t bytes);
inline const uint8_t* yk_dec_alpha_cur(const yk_ctx* c) { return c->dAlpha + (c->dAlphaBatch ? (size_t)c->dCur * c->dAlphaStride : 0); }
// yk_decode_compare_* (yk_quality.hip): the source of a comparison -- u8 pixels (planes == nullptr; CHW when planeBytes > 0) or int32 planes --
// and the two launches + one read-back over frames [firstFrame, firstFrame + nFrames) of the decode batch; the caller has validated and settled
struct YkQualitySrc {
    const uint8_t* src; size_t rowBytes, planeBytes; int srcChannels;
    const int32_t* const* planes; size_t strideElems;
    size_t frameStride;                                   // bytes (u8) or elements (int32) from one frame's source to the next
};
int yk_quality_compare(yk_ctx* c, const YkQualitySrc& q, int firstFrame, int nFrames, int channels, yk_quality* out, uint32_t* devTileSse);
void yk_dec_ring_free(yk_ctx* c);                         // the batch tables' pinned host ring and its events (yk_decode.hip)
void yk_dec_prepared_free(yk_ctx* c);                     // what yk_decode_prepare_device keeps (yk_decode.hip)
void yk_lut_dec_destroy(yk_ctx* c);                       // deletes the 3-D LUT decode tables and, below, the encoder's bank and streams (yk_lut3d.hip)
void yk_lut_destroy(yk_ctx* c);
int yk_pp_activate(yk_ctx* c);                           // per-plane coverage / corner flags for the passes behind the RGB passes
int yk_launch_encode2(yk_ctx* c, const YkEncodeParams& P);
int yk_qtab_get(yk_ctx* c);                              // builds the device's quantiser table on first use, sets c->qtab
void yk_selftest_qtab_launch(yk_ctx* c, int* mismatches);
