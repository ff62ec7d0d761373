// yk_stages.hip — the kernels around the fused encode kernel (yk_encode2.hip) and the stage launchers.
//
//   yk_alpha_kernel        a9   EncoderContext::MipPrefilter / quadRecursion   (encoder/EncoderContext.cpp:357-430, 1257-1427)
//   yk_scan*/yk_pack       stream compaction of the per-tile results into the reference's global streams
//                          (`streamTileDef` :4419, `streamTileIdx` :4421, nibble packing :1180-1184)
// The first-generation fused kernel (yk_encode_kernel: lane = one row of four pixels) is no longer part of this library: it lives in
// tests/csrc/yk_encode_v1.hip as an independent second implementation the parity tests cross-check against (yk_set_cross_check_launcher).
//
// No MFMA: integer / byte work bounded by HBM streaming.
#include "yk_common.h"
#ifdef YK_TEST_HOOKS
#include "../../include/yaik_hip_test.h"
#endif
#include "yk_device.h"

// ------------------------------------------------------------------------------------------------------------------
// a9: alpha tile-reject.  keep[mt] = 1 iff any of the 256 alphas of the aligned 16x16 block is non-zero (closed form of
// quadRecursion with maxMipLevel 3, EncoderContext.cpp:394-423); kept blocks grow the bounding box (boundingL/T/R/B, :416-422).
//
// Two kernels: yk_alpha_kernel decides the tiles, yk_alpha_box_kernel folds the image-wide box.  A work unit of yk_alpha_kernel is
// (YK_ALPHA_R rows of 16x16 tiles, 256-pixel segment) and belongs to ONE wave: the wave owns its tiles, so it writes their flags outright
// (nothing to clear) and knows their box.  The plane is read with 16-byte loads, a wave instruction covering 1 KB of one row; four adjacent
// lanes hold the 16 columns of one tile, a wave 16 tiles across.  One non-zero sample decides a tile, so a unit reads in two steps: every
// lane PROBES the first and the last row of each of its tiles (all 2 * YK_ALPHA_R probe loads of the unit in flight together, addresses
// clamped, no branch), one ballot per row of tiles gives the tiles already known to be kept, and only the lanes of tiles still undecided
// read the 14 rows in between: the rows of tiles that still hold an undecided tile are taken two at a time, 28 loads in flight before one
// wait.  A wave without an undecided tile issues nothing of the second step.  HBM serves 128-byte requests = the lanes of two adjacent
// tiles: an opaque region costs 2 of its 16 rows, a transparent one all 16.  The first and the last row are the two that the partly covered
// tiles along the top and the bottom of an opaque shape have in common with it (tiles along its sides are non-zero in every row); only a
// blob strictly inside a tile's rows 1..14 needs the second step to be kept.
// A wave only streams: it takes part in no protocol (no atomics, no wait for a store's acknowledgement, no barrier, no LDS) and ends after
// one to 1 + YK_ALPHA_R / 2 round trips.  The waves of a workgroup share nothing; how many there are decides WHEN the kernel runs beside
// the other frame's fused kernel (one-wave workgroups, 128 VGPRs, 4 waves per SIMD), because a workgroup starts once that many slots are
// free on one compute unit.  One-wave workgroups get every slot that kernel frees: they finish 130-160 us before it and lengthen it by
// 22 us for 11 us less gap behind it.  Two waves: 44 us before its end, +18 us.  Four or eight wait until it drains and end 23 us after it.
// Three do a part of the work under it (+3 us) and end 13 us after it: the shortest frame of what was measured (DESIGN 3.1,
// profiles/alpha_stream/variants.txt).
// The image-wide box: every unit leaves its box {x0, y0, x1, y1} ({9999999, 9999999, -1, -1} when it keeps nothing) in a slot of its own
// with a plain store -- every slot is rewritten by every launch, nothing is cleared between frames, every unit intersects the image -- and
// yk_alpha_box_kernel, one workgroup per frame right behind it on the stream, folds the slots into bounds[8..11] (stream order publishes them).
// ------------------------------------------------------------------------------------------------------------------
typedef int yk_i4 __attribute__((ext_vector_type(4)));
#ifndef YK_ALPHA_WAVES
#define YK_ALPHA_WAVES 3                                          // waves = units per workgroup; 1, 2, 3, 4 and 8 were measured
#endif
__global__ __launch_bounds__(64 * YK_ALPHA_WAVES, 4) void yk_alpha_kernel(const int32_t* __restrict__ alpha0, int strideElems, int w, int h, int y0,
                                                      uint8_t* __restrict__ keep0, int mtW, int mtH, unsigned long long planeStride,
                                                      unsigned long long keepStride, yk_i4* __restrict__ unitBox0, unsigned total) {
    const int lane = threadIdx.x & 63;
    const int vecPerRow = w >> 2;                                // int4 per image row (w is a multiple of 8)
    const int nSeg = (vecPerRow + 63) >> 6;                      // 64 int4 = 16 tiles per segment
    const int nUnits = nSeg * ((mtH + YK_ALPHA_R - 1) / YK_ALPHA_R);
    const unsigned uu = blockIdx.x * YK_ALPHA_WAVES + (threadIdx.x >> 6);        // wave = unit; units x frames in all
    if (uu >= total) return;
    const int f = (int)(uu / (unsigned)nUnits), u = (int)(uu - (unsigned)f * (unsigned)nUnits);
    const int32_t* alpha = alpha0 + (size_t)f * planeStride;
    uint8_t* keep = keep0 + (size_t)f * keepStride;
    const int tyU = u / nSeg, seg = u - tyU * nSeg, ty0 = tyU * YK_ALPHA_R;
    const int xv = seg * 64 + lane;
    const bool inX = xv < vecPerRow;
    const bool tileLane = (lane & 3) == 0;
    const int tx = xv >> 2;
    // ---- probe: rows 0 and 15 of every tile of the unit.  Addresses are clamped (column into the row, rows onto the image's last row) and
    // every lane loads: no load sits in a branch, all YK_ALPHA_R * 2 are in flight together; what a clamped lane read is masked afterwards.
    const int xvc = min(xv, vecPerRow - 1);
    uint32_t nzBits = 0, undBits = 0, rowsLeft = 0;              // bit r = row r of the unit's tiles: lane saw a sample / lane's tile undecided / (wave-uniform) some tile undecided
    {
        yk_i4 p[YK_ALPHA_R][2];
#pragma unroll
        for (int r = 0; r < YK_ALPHA_R; r++) {
            const int yA = min((ty0 + r) * 16, h - 1), yB = min(yA + 15, h - 1);
            p[r][0] = __builtin_nontemporal_load(reinterpret_cast<const yk_i4*>(alpha + (size_t)yA * strideElems + (size_t)xvc * 4));
            p[r][1] = __builtin_nontemporal_load(reinterpret_cast<const yk_i4*>(alpha + (size_t)yB * strideElems + (size_t)xvc * 4));
        }
#pragma unroll
        for (int r = 0; r < YK_ALPHA_R; r++) {
            const bool on = inX && (ty0 + r) * 16 < h;          // the lane's 4 columns and the tile's first row are inside the image
            const yk_i4 o = p[r][0] | p[r][1];
            const bool nz = ((o.x | o.y | o.z | o.w) != 0) & on;              // bitwise: the loads stay in front of every branch
            const unsigned long long pb = __ballot(nz);
            const bool und = on && ((pb >> (lane & ~3)) & 0xFULL) == 0;          // nothing seen in the tile's probed rows: rows 1..14 decide
            nzBits |= (nz ? 1u : 0u) << r; undBits |= (und ? 1u : 0u) << r;
            if (__ballot(und) != 0) rowsLeft |= 1u << r;
        }
    }
    // ---- the rows in between, for undecided tiles only, two rows of tiles at a time (the rows of tiles without an undecided tile are skipped:
    // a wave of decided tiles issues none of these instructions).  The 2 x 14 loads are issued under the lanes' masks and waited for once.
    while (rowsLeft) {
        const int rA = __ffs((int)rowsLeft) - 1; rowsLeft &= rowsLeft - 1;
        const bool two = rowsLeft != 0;
        const int rB = two ? __ffs((int)rowsLeft) - 1 : rA; rowsLeft &= rowsLeft - 1;
        yk_i4 a[2][14];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int r = j ? rB : rA, ty = ty0 + r;
            const bool und = (j == 0 || two) && ((undBits >> r) & 1u) != 0;
            const int32_t* col = alpha + (size_t)(ty * 16) * strideElems + (size_t)xv * 4;
#pragma unroll
            for (int k = 0; k < 14; k++) {
                a[j][k] = (yk_i4){0, 0, 0, 0};
                if (und && ty * 16 + 1 + k < h) a[j][k] = __builtin_nontemporal_load(reinterpret_cast<const yk_i4*>(col + (size_t)(1 + k) * strideElems));
            }
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            int m = 0;
#pragma unroll
            for (int k = 0; k < 14; k++) m |= a[j][k].x | a[j][k].y | a[j][k].z | a[j][k].w;
            nzBits |= (m != 0 ? 1u : 0u) << (j ? rB : rA);
        }
    }
    int colLo = 0x7FFFFFFF, colHi = -1, rowLo = 0x7FFFFFFF, rowHi = -1;          // wave-uniform: kept tile columns / rows of the unit
#pragma unroll
    for (int r = 0; r < YK_ALPHA_R; r++) {
        const int ty = ty0 + r;
        if (ty >= mtH) break;
        const unsigned long long b = __ballot(((nzBits >> r) & 1u) != 0);
        const bool kept = ((b >> (lane & ~3)) & 0xFULL) != 0;
        if (tileLane && tx < mtW) keep[(size_t)ty * mtW + tx] = kept ? 1 : 0;
        const unsigned long long kb64 = __ballot(tileLane && kept && tx < mtW);  // the kept tiles of this row of tiles
        if (kb64) {
            colLo = min(colLo, seg * 16 + ((__ffsll((long long)kb64) - 1) >> 2));
            colHi = max(colHi, seg * 16 + ((63 - __clzll((long long)kb64)) >> 2));
            rowLo = min(rowLo, ty); rowHi = max(rowHi, ty);
        }
    }
    if (lane == 0) {
        const bool any = colHi >= 0;
        unitBox0[(size_t)f * nUnits + u] = any ? (yk_i4){colLo * 16, y0 + rowLo * 16, colHi * 16 + 16, y0 + rowHi * 16 + 16} : (yk_i4){9999999, 9999999, -1, -1};
    }
}

// One workgroup per frame folds the frame's unit boxes into bounds[f * 16 + 8 .. 11] = {min x0, min y0, max x1, max y1} ({9999999, 9999999, -1, -1}
// when nothing is kept).  16 boxes per lane are in flight before a wait (the 4096 boxes of an 8192 x 8192 frame: one round trip -- as one wave
// with two round trips the kernel took 10-19 us beside the pack kernel of the other frame); an index past the last box reads the last box
// again, which changes no minimum and no maximum.
__global__ __launch_bounds__(256) void yk_alpha_box_kernel(const yk_i4* __restrict__ unitBox0, int nUnits, int32_t* __restrict__ bounds) {
    __shared__ yk_i4 s_box[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const yk_i4* ub = unitBox0 + (size_t)blockIdx.x * nUnits;
    int x0 = 9999999, gy0 = 9999999, x1 = -1, gy1 = -1;
    for (int base = 0; base < nUnits; base += 256 * 16) {
        yk_i4 v[16];
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = ub[min(base + j * 256 + (int)threadIdx.x, nUnits - 1)];
#pragma unroll
        for (int j = 0; j < 16; j++) { x0 = min(x0, v[j].x); gy0 = min(gy0, v[j].y); x1 = max(x1, v[j].z); gy1 = max(gy1, v[j].w); }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        x0 = min(x0, __shfl_xor(x0, d)); x1 = max(x1, __shfl_xor(x1, d));
        gy0 = min(gy0, __shfl_xor(gy0, d)); gy1 = max(gy1, __shfl_xor(gy1, d));
    }
    if (lane == 0) s_box[wv] = (yk_i4){x0, gy0, x1, gy1};
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < 4; k++) { x0 = min(x0, s_box[k].x); gy0 = min(gy0, s_box[k].y); x1 = max(x1, s_box[k].z); gy1 = max(gy1, s_box[k].w); }
        *reinterpret_cast<yk_i4*>(bounds + (size_t)blockIdx.x * 16 + 8) = (yk_i4){x0, gy0, x1, gy1};
    }
}

// test path only (the first-generation cross-check kernel reads the published form): bounds[0..3] = the box, bounds[4] = "bbox == whole image ->
// every reject discarded" (EncoderContext.cpp:1294, :1400-1403).  The library's own kernel derives the flag from the box.
__global__ void yk_alpha_publish_kernel(int32_t* __restrict__ bounds, int srcOff, int fullW, int fullH) {
    bounds += (size_t)blockIdx.x * 16;
    const int b0 = bounds[srcOff], b1 = bounds[srcOff + 1], b2 = bounds[srcOff + 2], b3 = bounds[srcOff + 3];
    bounds[0] = b0; bounds[1] = b1; bounds[2] = b2; bounds[3] = b3;
    bounds[4] = (b0 == 0 && b1 == 0 && b2 == fullW && b3 == fullH) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------
// stream compaction: per-tile (count, def, 32-byte nibble slot) -> the reference's global streams, LeftRightOrder =
// row-major over the tile grid (tiles outside the constraint box carry count 0).
// ------------------------------------------------------------------------------------------------------------------
#define YK_SCAN_TILE 1024

// first scan level for the first-generation kernel (the second-generation kernel accumulates these sums itself)
__global__ __launch_bounds__(1024) void yk_scan1_kernel(const uint8_t* __restrict__ tileCount, size_t T8, uint32_t* __restrict__ blockCnt) {
    __shared__ uint32_t s_tmp[32];
    const size_t i = (size_t)blockIdx.x * YK_SCAN_TILE + threadIdx.x;
    const uint32_t c = (i < T8) ? tileCount[i] : 0;                          // plane 0: the counts do not depend on the plane
    uint32_t tot2, totN;
    yk_block_exscan(c ? 1u : 0u, s_tmp, &tot2);
    yk_block_exscan(c, s_tmp, &totN);
    if (threadIdx.x == 0) { blockCnt[(size_t)blockIdx.x * 2] = totN; blockCnt[(size_t)blockIdx.x * 2 + 1] = tot2; }
}

// second level: exclusive prefix over the per-block sums (consumed and cleared for the next frame) and the totals of the
// three planes (identical: the counts do not depend on the plane).  One workgroup of 1024 threads.
__device__ __forceinline__ void yk_scan2_body(uint32_t* __restrict__ blockCnt, uint32_t* __restrict__ blockSums, int nBlocks, uint32_t* __restrict__ totals, uint32_t* s_tmp) {
    uint32_t baseN = 0, baseD = 0;
    for (int start = 0; start < nBlocks; start += 1024) {
        const int i = start + threadIdx.x;
        const uint32_t n = i < nBlocks ? blockCnt[i * 2] : 0, d = i < nBlocks ? blockCnt[i * 2 + 1] : 0;
        uint32_t totN, totD;
        const uint32_t en = yk_block_exscan(n, s_tmp, &totN);
        const uint32_t ed = yk_block_exscan(d, s_tmp, &totD);
        if (i < nBlocks) {
            blockSums[i * 2] = baseN + en; blockSums[i * 2 + 1] = baseD + ed;
            blockCnt[i * 2] = 0; blockCnt[i * 2 + 1] = 0;
        }
        baseN += totN; baseD += totD;
    }
    if (threadIdx.x < 3) { totals[threadIdx.x * 2] = baseD; totals[threadIdx.x * 2 + 1] = baseN; }
}
__global__ __launch_bounds__(1024) void yk_scan2_kernel(uint32_t* __restrict__ blockCnt, uint32_t* __restrict__ blockSums, int nBlocks,
                                                        uint32_t* __restrict__ totals, unsigned long long blockNStride) {
    __shared__ uint32_t s_tmp[32];
    yk_scan2_body(blockCnt + (size_t)blockIdx.x * blockNStride, blockSums + (size_t)blockIdx.x * blockNStride, nBlocks, totals + (size_t)blockIdx.x * 8, s_tmp);   // blockIdx.x = frame of a batch
}

// first level for the second-generation fused kernel, which neither adds to shared counters nor ORs into a shared map (atomics on one address are
// served one after the other and were 15-23 % of that kernel on noisy frames): every strip leaves the sums of its two runs of eight tiles in words
// of their own (runSums: nibbles / 16 | coded tiles << 16) and its four 16x16 bits in a byte of its own (bm0b).  Here the 128 run words of a scan
// block = 32 consecutive 16-byte pieces = one half-wave are added into the block's two counters (plain stores: nothing to clear, every word is
// rewritten every frame), and the four bytes of a 64x64 block are folded into its 16-bit word of the 16x16 map.
__global__ __launch_bounds__(1024) void yk_scan1r_kernel(const uint32_t* __restrict__ runSums, unsigned long long runStride, int nRuns,
                                                         uint32_t* __restrict__ blockCnt, unsigned long long blockNStride, int nBlocks,
                                                         const uint8_t* __restrict__ bm0b, unsigned long long bm0bStride, uint8_t* __restrict__ bitmap0,
                                                         unsigned long long bitmap0Stride, int nB64) {
    const size_t f = blockIdx.y;                                                  // frame of a batch
    const int g = (int)blockIdx.x * 1024 + (int)threadIdx.x;
    if (runSums) {
        const uint4* rs4 = reinterpret_cast<const uint4*>(runSums + f * runStride);
        const int n4 = (nRuns + 3) >> 2;                                          // the array is padded with zero words to a multiple of four
        const uint4 v = g < n4 ? rs4[g] : make_uint4(0u, 0u, 0u, 0u);
        uint32_t acc = v.x + v.y + v.z + v.w;                                     // both 16-bit halves at once: at most 128 x 32 and 128 x 8 per block
        acc += __shfl_xor(acc, 16, 32); acc += __shfl_xor(acc, 8, 32); acc += __shfl_xor(acc, 4, 32); acc += __shfl_xor(acc, 2, 32); acc += __shfl_xor(acc, 1, 32);
        const int blk = g >> 5;
        if ((threadIdx.x & 31) == 0 && blk < nBlocks) {
            uint2* dst = reinterpret_cast<uint2*>(blockCnt + f * blockNStride) + blk;
            *dst = make_uint2(16u * (acc & 0xFFFFu), acc >> 16);
        }
    }
    if (g < nB64) {
        const uint32_t b = reinterpret_cast<const uint32_t*>(bm0b + f * bm0bStride)[g];   // the four strips' bytes of block g, 4 bits each
        uint16_t* dst = reinterpret_cast<uint16_t*>(bitmap0 + f * bitmap0Stride);
        dst[g] = (uint16_t)((b & 0xFu) | ((b >> 4) & 0xF0u) | ((b >> 8) & 0xF00u) | ((b >> 12) & 0xF000u));
        if (g == nB64 - 1 && (nB64 & 1)) dst[nB64] = 0;                           // the padding half of the last 32-bit word (word-wise consumers)
    }
}

// One workgroup of four waves packs the nibbles of 1024 consecutive tiles, the three planes one after the other: a tile's count is the same in the
// three planes, so ONE scan serves them all, and it is a scan of one packed word per tile (nibbles | coded << 16: at most 1023 x 64 and 1023 in
// front of a tile, no carry between the halves).  A lane holds four consecutive tiles (two 16-byte loads of their records), so the scan is a
// wave scan of the lanes' sums plus three words across the waves.  Every tile holds a multiple of 16 nibbles (16 per uncovered 4x4 quadrant),
// so every stream offset is a multiple of 8 bytes: after the scan two lanes per tile copy the halves of its slot straight to their place in
// the stream, 16 bytes at a time where the half is whole and 8 where it is not, reading only the bytes that exist.  256 threads, because a
// workgroup of 1024 needs 16 free wave slots on ONE compute unit and waits for them while a fused kernel holds the chip.
struct __attribute__((aligned(8))) YkPiece16 { uint32_t a, b, c, d; };           // 16 bytes at an 8-byte aligned place of a stream
__global__ __launch_bounds__(256) void yk_pack_kernel(const uint8_t* __restrict__ tileCount, const uint16_t* __restrict__ tileDef, const uint2* __restrict__ tileInfo,
                                                      const uint8_t* __restrict__ slots, size_t T8, const uint32_t* __restrict__ blockSums, int nBlocks,
                                                      uint16_t* __restrict__ defsOut, uint32_t* __restrict__ nibOut, size_t nibStrideWords, YkFrameStrides fs,
                                                      const uint32_t* __restrict__ blockCnt, uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_wave[4];
    __shared__ unsigned long long s_pre;
    __shared__ uint32_t s_off[YK_SCAN_TILE];
    __shared__ uint8_t s_cnt[YK_SCAN_TILE];
    {   // blockIdx.z = frame of a batch
        const size_t f = blockIdx.z;
        tileCount += f * fs.tileCount; tileDef += f * fs.tileDef; slots += f * fs.slots; blockSums += f * fs.blockN;
        if (tileInfo) tileInfo += f * fs.tileInfo;
        defsOut += f * fs.defsOut; nibOut += f * (fs.nibOut / 4);
        if (blockCnt) { blockCnt += f * fs.blockN; totals += f * 8; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i0 = (size_t)blockIdx.x * YK_SCAN_TILE, i = i0 + (size_t)threadIdx.x * 4;
    // second-generation fused kernel: one record per tile {def0 | def1 << 16, def2 | count << 16}; first generation: count and definition arrays
    uint32_t c[4] = {0, 0, 0, 0}, d01[4] = {0, 0, 0, 0}, d2[4] = {0, 0, 0, 0};
    if (tileInfo && i + 4 <= T8) {
        const uint4 r0 = reinterpret_cast<const uint4*>(tileInfo + i)[0], r1 = reinterpret_cast<const uint4*>(tileInfo + i)[1];   // i is a multiple of 4, a frame starts at a multiple of 16 bytes
        d01[0] = r0.x; c[0] = r0.y >> 16; d2[0] = r0.y & 0xFFFFu; d01[1] = r0.z; c[1] = r0.w >> 16; d2[1] = r0.w & 0xFFFFu;
        d01[2] = r1.x; c[2] = r1.y >> 16; d2[2] = r1.y & 0xFFFFu; d01[3] = r1.z; c[3] = r1.w >> 16; d2[3] = r1.w & 0xFFFFu;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i + j >= T8) continue;
            if (tileInfo) { const uint2 ti = tileInfo[i + j]; c[j] = ti.y >> 16; d01[j] = ti.x; d2[j] = ti.y & 0xFFFFu; }
            else { c[j] = tileCount[i + j]; if (c[j]) { d01[j] = (uint32_t)tileDef[i + j] | ((uint32_t)tileDef[T8 + i + j] << 16); d2[j] = tileDef[2 * T8 + i + j]; } }
        }
    }
    // Second scan level inside this kernel (second-generation fused kernel: the per-block sums come from yk_scan1r_kernel): ONE wave adds the sums
    // of the blocks in front of this one (at most 8 KB from L2, 16 independent loads per lane) while the others scan; nobody waits for another
    // workgroup or for a one-workgroup kernel in the frame's chain of launches.
    if (blockCnt && wave == 3) {
        unsigned long long acc = 0;                                               // coded tiles << 32 | nibbles
        for (int k = lane; k < (int)blockIdx.x; k += 64) { const uint2 v = reinterpret_cast<const uint2*>(blockCnt)[k]; acc += ((unsigned long long)v.y << 32) | v.x; }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) s_pre = acc;
    }
    uint32_t w[4], mine = 0;                                                      // the packed word of each tile, exclusive inside the lane
#pragma unroll
    for (int j = 0; j < 4; j++) { w[j] = mine; mine += c[j] | (c[j] ? 0x10000u : 0u); }
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d); if (lane >= d) incl += o; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t front = incl - mine;                                                 // tiles of this workgroup in front of the lane's
#pragma unroll
    for (int k = 0; k < 3; k++) if (k < wave) front += s_wave[k];
    uint32_t baseN, baseD;
    if (blockCnt) {
        baseN = (uint32_t)s_pre; baseD = (uint32_t)(s_pre >> 32);
        if (blockIdx.x == (unsigned)nBlocks - 1 && threadIdx.x < 3) {            // the totals of the three planes (identical)
            const uint2 v = reinterpret_cast<const uint2*>(blockCnt)[nBlocks - 1];
            totals[threadIdx.x * 2] = baseD + v.y; totals[threadIdx.x * 2 + 1] = baseN + v.x;
        }
    } else { baseN = blockSums[(size_t)blockIdx.x * 2]; baseD = blockSums[(size_t)blockIdx.x * 2 + 1]; }     // same for the three planes
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t e = front + w[j], en = e & 0xFFFFu, ed = e >> 16;
        s_off[threadIdx.x * 4 + j] = (baseN + en) >> 1;                           // byte offset inside a plane's stream
        s_cnt[threadIdx.x * 4 + j] = (uint8_t)c[j];
        if (c[j]) { defsOut[baseD + ed] = (uint16_t)d01[j]; defsOut[T8 + baseD + ed] = (uint16_t)(d01[j] >> 16); defsOut[2 * T8 + baseD + ed] = (uint16_t)d2[j]; }
    }
    __syncthreads();
    const int half = threadIdx.x & 1;
#pragma unroll
    for (int p = 0; p < 3; p++) {
        uint8_t* out = reinterpret_cast<uint8_t*>(nibOut + (size_t)p * nibStrideWords);
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int t = it * 128 + (threadIdx.x >> 1);
            const size_t ti = i0 + t;
            const int left = (s_cnt[t] >> 1) - half * 16;                         // bytes of this half: a multiple of 8 (tiles past T8 hold 0)
            const uint8_t* src = slots + ((size_t)p * T8 + ti) * YK_SLOT + half * 16;
            uint8_t* dst = out + s_off[t] + half * 16;
            if (left >= 16) { const uint4 v = *reinterpret_cast<const uint4*>(src); *reinterpret_cast<YkPiece16*>(dst) = YkPiece16{v.x, v.y, v.z, v.w}; }
            else if (left >= 8) *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------------------------
// test hook: the launcher of an independent second implementation of the fused kernel (same YkEncodeParams, same outputs)
static int (*g_crossCheckLauncher)(hipStream_t, const YkEncodeParams*) = nullptr;
#ifdef YK_TEST_HOOKS
extern "C" int yk_set_cross_check_launcher(void* fn) { g_crossCheckLauncher = reinterpret_cast<int (*)(hipStream_t, const YkEncodeParams*)>(fn); return YK_OK; }
#endif

int yk_launch_alpha(yk_ctx* c, bool batch) {
    const int F = batch ? c->nFrames : 1;
    const YkFrameView V = yk_frame(c, batch ? 0 : c->curFrame);   // a batch launch starts at frame 0 and strides on by fs
    const long long nUnits = (long long)yk_alpha_units(c->fullW, c->mtH);
    if (nUnits * F > 0x7FFFFFFFLL) return yk_fail(c, YK_ERR_BAD_ARG, "too many alpha work units for one launch");
    yk_i4* unitBox = reinterpret_cast<yk_i4*>(static_cast<int*>(c->img.alphaUnitBox));
    // never fewer waves than units: nothing loops, a wave ends after its unit
    hipLaunchKernelGGL(yk_alpha_kernel, dim3((unsigned)((nUnits * F + YK_ALPHA_WAVES - 1) / YK_ALPHA_WAVES)), dim3(64 * YK_ALPHA_WAVES), 0, c->stream, V.plane[3], c->strideElems,
                       c->fullW, c->h, c->y0, V.keep, c->mtW, c->mtH, (unsigned long long)c->fs.plane, (unsigned long long)c->fs.keep, unitBox, (unsigned)(nUnits * F));
    hipLaunchKernelGGL(yk_alpha_box_kernel, dim3((unsigned)F), dim3(256), 0, c->stream, unitBox, (int)nUnits, V.bounds);
    YK_HIP(c, hipGetLastError());
    c->boundsOff = 8;                                           // whole image / batch: the accumulators are the box; a stripe caller replaces it (yk_alpha_finish)
    return YK_OK;
}

int yk_launch_alpha_finish(yk_ctx* c, const int32_t* globalBBox) {
    // whole image: the box is where yk_alpha_kernel accumulated it; stripes: the host-combined box goes to bounds[0..4]
    if (globalBBox) {
        int32_t b[5] = { globalBBox[0], globalBBox[1], globalBBox[2], globalBBox[3], 0 };
        b[4] = (b[0] == 0 && b[1] == 0 && b[2] == c->fullW && b[3] == c->fullH) ? 1 : 0;
        YK_HIP(c, hipMemcpyAsync(yk_frame(c).bounds, b, sizeof b, hipMemcpyHostToDevice, c->stream));
        c->boundsOff = 0;
    }
    return YK_OK;
}

int yk_launch_encode(yk_ctx* c, int rejectFactor, int mode3BitOnly, int wantDst, bool batch) {
    const YkFrameView V = yk_frame(c, batch ? 0 : c->curFrame);   // a batch launch starts at frame 0 and strides on by fs
    YkEncodeParams P;
    for (int i = 0; i < 4; i++) P.plane[i] = V.plane[i];
    P.strideElems = c->strideElems; P.w = c->fullW; P.h = c->h; P.hAvail = c->h + c->halo; P.y0 = c->y0; P.fullH = c->fullH;
    P.rejectFactor = rejectFactor; P.startMode = mode3BitOnly ? 3 : 0; P.wantDst = wantDst; P.ablate = c->ablate;
    P.keep = (c->nPlanes == 4) ? V.keep : nullptr;
    P.bounds = (c->nPlanes == 4) ? V.bounds + c->boundsOff : nullptr;   // {x0, y0, x1, y1}; the kernel derives the discard rule
    for (int i = 0; i < 7; i++) P.bitmap[i] = V.bitmap[i];
    P.coverage = V.coverage; P.tileDef = V.tileDef; P.tileCount = V.tileCount; P.slots = V.slots;
    P.blockCnt = c->kernelVersion == 2 ? V.blockCnt : nullptr;
    for (int i = 0; i < 3; i++) P.dst[i] = c->img.dst[i];
    P.tilesW = c->tilesW; P.tilesH = c->tilesH; P.mtW = c->mtW; P.mtH = c->mtH;
    P.xBB64 = (c->fullW + 63) / 64; P.yBB64 = (c->h + 63) / 64; P.xBB32 = (c->fullW + 31) / 32; P.yBB32 = (c->h + 31) / 32;
    P.nFrames = batch ? c->nFrames : 1; P.fs = c->fs;
    P.qtab = c->qtab;
    P.small = V.small;                                          // the view's arrays of the small-output arena, as byte offsets into it
    auto off = [&](const void* p) { return (uint32_t)(static_cast<const uint8_t*>(p) - V.small); };
    for (int i = 0; i < 7; i++) P.oBm[i] = off(V.bitmap[i]);
    P.oBm0b = off(V.bm0b); P.oCov = off(V.coverage); P.oInfo = off(V.tileInfo); P.oRun = off(V.runSums);
    P.divXBB64 = c->divXBB64; P.divNBf = c->divNBf;
    P.outTab = c->img.outTab; P.outFrame0 = batch ? 0u : (uint32_t)c->curFrame;    // the table holds frame 0's offsets
    P.pixCache = nullptr; c->pixCacheValid = false;
    if (c->pixCacheOn && !batch && c->kernelVersion == 2 && c->nFrames == 1) {
        if (!c->img.pixCache) YK_HIP(c, c->img.pixCache.alloc(c->stream, (size_t)P.xBB64 * 64 * ((size_t)(c->h + 15) / 16 * 16) / 4, 4096));
        P.pixCache = c->img.pixCache; c->pixCacheValid = true;
    }
    if (c->kernelVersion == 2) return yk_launch_encode2(c, P);
    // version 1 = the cross-check implementation of the test suite (tests/csrc/yk_encode_v1.hip), registered at run time
    if (batch) return yk_fail(c, YK_ERR_STATE, "batches need kernel version 2");
    if (c->nPlanes == 4) {                                      // it reads the published form bounds[0..4]
        hipLaunchKernelGGL(yk_alpha_publish_kernel, dim3(1), dim3(1), 0, c->stream, V.bounds, c->boundsOff, c->fullW, c->fullH);
        P.bounds = V.bounds;
    }
    if (!g_crossCheckLauncher) return yk_fail(c, YK_ERR_STATE, "kernel version 1 is not part of this library: register it with yk_set_cross_check_launcher");
    if (g_crossCheckLauncher(c->stream, &P) != 0) return yk_fail(c, YK_ERR_HIP, "cross-check kernel launch", hipGetLastError());
    return YK_OK;
}

int yk_launch_pack(yk_ctx* c, bool batch) {
    const size_t T8 = (size_t)c->tilesW * c->tilesH;
    const int nb = c->nScanBlocks, F = batch ? c->nFrames : 1;
    const YkFrameView V = yk_frame(c, batch ? 0 : c->curFrame);   // a batch launch starts at frame 0 and strides on by fs
    if (c->kernelVersion != 2) hipLaunchKernelGGL(yk_scan1_kernel, dim3(nb), dim3(1024), 0, c->stream, V.tileCount, T8, V.blockCnt);
    // second-generation fused kernel: per-run sums and per-strip 16x16 bytes instead of atomics, per-tile records instead of count / definition arrays
    const bool v2 = c->kernelVersion == 2;
    const uint32_t* runSums = (v2 && (c->tilesW & 7) == 0) ? V.runSums : nullptr;
    const uint8_t* bm0b = v2 ? V.bm0b : nullptr;
    const uint2* tileInfo = v2 ? V.tileInfo : nullptr;
    const int nB64 = ((c->fullW + 63) / 64) * ((c->h + 63) / 64);
    if (v2) {
        const int nRuns = (int)((T8 + 7) / 8), n4 = (nRuns + 3) >> 2;
        const int items = runSums ? (n4 > nB64 ? n4 : nB64) : nB64;
        hipLaunchKernelGGL(yk_scan1r_kernel, dim3((unsigned)((items + 1023) / 1024), F), dim3(1024), 0, c->stream, runSums, (unsigned long long)c->fs.runSums, nRuns,
                           V.blockCnt, (unsigned long long)c->fs.blockN, nb, bm0b, (unsigned long long)c->fs.bm0b,
                           V.bitmap[0], (unsigned long long)c->fs.bitmap[0], nB64);
    }
    if (!runSums) hipLaunchKernelGGL(yk_scan2_kernel, dim3(F), dim3(1024), 0, c->stream, V.blockCnt, V.blockSums, nb, V.totals, (unsigned long long)c->fs.blockN);
    hipLaunchKernelGGL(yk_pack_kernel, dim3(nb, 1, F), dim3(256), 0, c->stream, V.tileCount, V.tileDef, tileInfo,
                       V.slots, T8, V.blockSums, nb, V.defsOut, reinterpret_cast<uint32_t*>(V.nibOut), c->nibStride / 4, c->fs,
                       runSums ? V.blockCnt : (const uint32_t*)nullptr, V.totals);
    YK_HIP(c, hipGetLastError());
    return YK_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// self-test hooks (run by tests/test_gpu_selftest.py): exhaustive checks of the arithmetic shortcuts used above
// ------------------------------------------------------------------------------------------------------------------
__global__ void yk_selftest_div_kernel(int* mismatches) {
    const int n = blockIdx.x, d = threadIdx.x + 1;           // n in 0..255, d in 1..256
    const float fn = (float)n, fd = (float)d;
    const float ref = __fdiv_rn(fn, fd);
    const float got = yk_div_exact(fn, fd, __fdiv_rn(1.0f, fd));
    if (__float_as_uint(ref) != __float_as_uint(got)) atomicAdd(mismatches, 1);
}

__global__ void yk_selftest_scale_kernel(int* mismatches) {
    const int scale = blockIdx.x + 1, d8 = threadIdx.x;        // scale 1..256 (superset of 3..223), d8 32..255
    if (d8 < 32) return;
    const int dnum = (d8 - 32) * 127 + (scale - 1);
    const int ref = dnum / scale;
    const int got = __float2int_rz(((float)dnum + 0.5f) * __builtin_amdgcn_rcpf((float)scale));
    if (ref != got) atomicAdd(mismatches, 1);
}

__global__ void yk_selftest_r1div_kernel(int* mismatches) {
    const int n = blockIdx.x * 16 + (threadIdx.x >> 4), d0 = (threadIdx.x & 15) * 16;     // n 0..4095, d 1..255
    for (int k = 0; k < 16; k++) {
        const int d = d0 + k;
        if (d < 1 || d > 255) continue;
        const int got = __float2int_rz(((float)n + 0.5f) * __builtin_amdgcn_rcpf((float)d));
        if (got != n / d) atomicAdd(mismatches, 1);
    }
}

// yk_r1_magic against the C expression of GetValueModel1 for every delta, minCol and pixel value the 1-D path can meet
__global__ void yk_selftest_r1magic_kernel(int* mismatches) {
    const int delta = blockIdx.x, x = threadIdx.x;               // delta 0..255, x = v - minCol 0..delta
    if (x > delta) return;
    for (int minCol = 0; minCol + delta <= 255; minCol++) {
        uint32_t A, B;
        yk_r1_magic(delta, minCol, &A, &B);
        const int v = minCol + x;
        int idx = 0;
        if (delta) { const int n = (v - minCol) * 15 + (delta >> 1) - 1; idx = n < 0 ? -1 : n / delta; }
        const uint32_t got = (__umul24((uint32_t)v, A) + B) >> 20;
        if (got != (uint32_t)(1 + idx)) atomicAdd(mismatches, 1);
    }
}

#ifdef YK_TEST_HOOKS
extern "C" int yk_selftest(yk_ctx* c, int which, int* result) {
    if (!c || !result) return YK_ERR_BAD_ARG;
    YK_HIP(c, hipSetDevice(c->device));
    YkBuf<int> d;
    YK_HIP(c, d.alloc(c->stream, 1));
    YK_HIP(c, hipMemsetAsync(d, 0, sizeof(int), c->stream));
    if (which == 0) hipLaunchKernelGGL(yk_selftest_div_kernel, dim3(256), dim3(256), 0, c->stream, d);
    else if (which == 1) hipLaunchKernelGGL(yk_selftest_scale_kernel, dim3(256), dim3(256), 0, c->stream, d);
    else if (which == 2) hipLaunchKernelGGL(yk_selftest_r1div_kernel, dim3(256), dim3(256), 0, c->stream, d);
    else if (which == 3) yk_selftest_qtab_launch(c, d);
    else if (which == 4) hipLaunchKernelGGL(yk_selftest_r1magic_kernel, dim3(256), dim3(256), 0, c->stream, d);
    else return yk_fail(c, YK_ERR_BAD_ARG, "unknown selftest");
    YK_HIP(c, hipMemcpyAsync(result, d, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}
#endif
