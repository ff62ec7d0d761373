// yk_quality.hip — round-trip quality on the device: the decoder's 8x8-tiled u8 planes (and the decoded 'ALPM' plane) against a source image
// that is read where it lies.  Exact integer statistics per frame and channel: sse = sum (dec - src)^2, sad = sum |dec - src|, nDiff = samples
// that differ, maxAbs; optionally the SSE of every 8x8 tile.  Integers only: the result does not depend on summation order.
//
// Work unit = that of yk_dec_detile_kernel (yk_decode.hip, the comment above YK_DT_THREADS): 16 consecutive tiles, lane l loads bytes 16l..16l+15
// of each plane = rows 2(l&3), 2(l&3)+1 of tile 16u + (l>>2), so the plane reads are dense 1 KB accesses; a workgroup of four waves takes four
// units per wave (256 tiles), and a lane issues the loads of YK_Q_INFLIGHT units before it uses them.
// Sources: HWC u8 at src[y * rowBytes + x * srcChannels + k], CHW u8 at src[k * planeBytes + y * rowBytes + x], or int32 planes in the encoder's
// layout, plane[k][y * strideElems + x], low byte taken as the fused kernel does.  The source is read through byte pointers (__builtin_memcpy),
// so any base address and pitch is accepted with no alignment assumed.
//
// Reduction, no atomics anywhere: u32 accumulators per lane -> xor shuffles across the wave -> LDS across the four waves -> ONE record of 16
// u32 per workgroup, written with plain vector stores to partials[frame][workgroup]; yk_quality_fold_kernel (one workgroup per frame) folds the
// records into u64.
// BOUND of the u32 partials: a workgroup compares at most 256 lanes x 4 units x 16 pixels = 16384 samples per channel, so its sse is at most
// 16384 x 255^2 = 1 065 369 600 < 2^32 (sad and nDiff are smaller); a tile's SSE over four channels is at most 64 x 4 x 255^2 < 2^24.
// The FOLD is u64: a frame of 32760 x 32760 reaches 2^30 x 255^2 < 2^46.
#include "yk_common.h"
#include <vector>

#define YK_Q_THREADS 256
#define YK_Q_UNITS 4                                    // units per lane and workgroup
#define YK_Q_TILES (YK_Q_THREADS / 4 * YK_Q_UNITS)      // tiles per workgroup
#define YK_Q_REC 16                                     // u32 per record: [channel][sse, sad, nDiff, maxAbs]
#ifndef YK_Q_INFLIGHT_U8
#define YK_Q_INFLIGHT_U8 YK_Q_UNITS                        // units an 8-bit source's lane loads before it uses the first (A/B builds: 2)
#endif

enum { YK_Q_HWC3 = 0, YK_Q_HWC4 = 1, YK_Q_CHW = 2, YK_Q_PLANES = 3 };

struct YkQArgs {
    const uint8_t* planes; size_t planeSize, planesFrame;   // decoded R, G, B of frame f at planes + f * planesFrame + p * planeSize
    const uint8_t* alpha; size_t strideA, alphaFrame;       // decoded alpha (four channels): row y of frame f at alpha + f * alphaFrame + y * strideA
    const uint8_t* src; size_t rowBytes, planeBytes;        // u8 source; frame f at src + f * srcFrame bytes
    const int32_t* sp[4]; size_t strideElems;               // int32 source planes; frame f at sp[k] + f * srcFrame elements
    size_t srcFrame;
    uint32_t tileW, nTiles;
    uint32_t* partials;                                     // [frame][gridDim.x][YK_Q_REC]
    uint32_t* tileMap;                                      // nullptr, or [frame][nTiles]
};

typedef uint32_t yk_q4 __attribute__((ext_vector_type(4)));

template <int CH, int L> struct YkQTraits {
    static constexpr int C = L == YK_Q_HWC3 ? 3 : 4;                                                   // bytes per source pixel (HWC)
    static constexpr int SRC = L == YK_Q_PLANES ? CH * 16 : L == YK_Q_CHW ? CH * 4 : 4 * C;            // source dwords a lane holds per unit
    static constexpr int INFLIGHT = L == YK_Q_PLANES ? 1 : YK_Q_INFLIGHT_U8;                                 // units loaded before the first is used
};
#define YK_Q_INFLIGHT(CH, L) (YkQTraits<CH, L>::INFLIGHT)

template <int CH, int L> struct YkQUnit { uint32_t d[3][4]; uint32_t a[4]; uint32_t s[YkQTraits<CH, L>::SRC]; };

template <int CH, int L>
__device__ __forceinline__ void yk_q_load(const YkQArgs& a, uint32_t t, uint32_t rp, YkQUnit<CH, L>& u) {
    const size_t ti = (size_t)t * 64 + rp * 16;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const yk_q4 v = *reinterpret_cast<const yk_q4*>(a.planes + k * a.planeSize + ti);
        u.d[k][0] = v.x; u.d[k][1] = v.y; u.d[k][2] = v.z; u.d[k][3] = v.w;
    }
    const uint32_t ty = t / a.tileW, tx = t - ty * a.tileW;
    const size_t y = (size_t)ty * 8 + rp * 2, x = (size_t)tx * 8;
    if constexpr (CH == 4) {
        __builtin_memcpy(&u.a[0], a.alpha + y * a.strideA + x, 8);
        __builtin_memcpy(&u.a[2], a.alpha + (y + 1) * a.strideA + x, 8);
    }
    if constexpr (L == YK_Q_PLANES) {
#pragma unroll
        for (int k = 0; k < CH; k++)
#pragma unroll
            for (int r = 0; r < 2; r++) __builtin_memcpy(&u.s[(k * 2 + r) * 8], a.sp[k] + (y + r) * a.strideElems + x, 32);
    } else if constexpr (L == YK_Q_CHW) {
#pragma unroll
        for (int k = 0; k < CH; k++)
#pragma unroll
            for (int r = 0; r < 2; r++) __builtin_memcpy(&u.s[(k * 2 + r) * 2], a.src + k * a.planeBytes + (y + r) * a.rowBytes + x, 8);
    } else {
        constexpr int C = YkQTraits<CH, L>::C;
#pragma unroll
        for (int r = 0; r < 2; r++) __builtin_memcpy(&u.s[r * 2 * C], a.src + (y + r) * a.rowBytes + x * C, 8 * C);
    }
}

// the lane's 16 pixels of one unit into its accumulators acc[channel][sse, sad, nDiff, maxAbs]; returns their SSE over the compared channels
template <int CH, int L>
__device__ __forceinline__ uint32_t yk_q_accumulate(const YkQUnit<CH, L>& u, uint32_t (&acc)[4][4]) {
    constexpr int C = YkQTraits<CH, L>::C;
    uint32_t before = 0, after = 0;
#pragma unroll
    for (int k = 0; k < CH; k++) before += acc[k][0];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int k = 0; k < CH; k++) {
                const uint32_t dw = k < 3 ? u.d[k][r * 2 + (j >> 2)] : u.a[r * 2 + (j >> 2)];
                const uint32_t dv = (dw >> (8 * (j & 3))) & 255u;
                uint32_t sv;
                if constexpr (L == YK_Q_PLANES) sv = u.s[(k * 2 + r) * 8 + j] & 255u;
                else if constexpr (L == YK_Q_CHW) sv = (u.s[(k * 2 + r) * 2 + (j >> 2)] >> (8 * (j & 3))) & 255u;
                else { const int b = j * C + k; sv = (u.s[r * 2 * C + (b >> 2)] >> (8 * (b & 3))) & 255u; }
                const uint32_t ad = __builtin_amdgcn_sad_u16(dv, sv, 0u);          // |dv - sv|: both below 2^16, the high halves are 0
                acc[k][0] += __umul24(ad, ad);                                     // ad <= 255: one 24-bit multiply-add
                acc[k][1] += ad;
                acc[k][2] += ad ? 1u : 0u;
                acc[k][3] = ad > acc[k][3] ? ad : acc[k][3];
            }
#pragma unroll
    for (int k = 0; k < CH; k++) after += acc[k][0];
    return after - before;
}

// the four lanes that hold a tile are a quad: its SSE by two quad permutes, one lane stores it
__device__ __forceinline__ void yk_q_tile_store(uint32_t* tileMap, uint32_t t, uint32_t rp, uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1, 0, 3, 2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2, 3, 0, 1]
    if (rp == 0) tileMap[t] = v;
}

template <int CH, int L>
__global__ __launch_bounds__(YK_Q_THREADS) void yk_quality_compare_kernel(YkQArgs a) {
    __shared__ uint32_t s_rec[YK_Q_THREADS / 64][YK_Q_REC];
    constexpr int KF = YkQTraits<CH, L>::INFLIGHT;
    const uint32_t f = blockIdx.y, bx = blockIdx.x;
    a.planes += (size_t)f * a.planesFrame;
    if constexpr (CH == 4) a.alpha += (size_t)f * a.alphaFrame;
    if constexpr (L == YK_Q_PLANES) {
#pragma unroll
        for (int k = 0; k < CH; k++) a.sp[k] += (size_t)f * a.srcFrame;
    } else a.src += (size_t)f * a.srcFrame;
    uint32_t* const tileMap = a.tileMap ? a.tileMap + (size_t)f * a.nTiles : nullptr;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rp = lane & 3;
    // unit of step k: bx * 16 + k * 4 + wave, as in yk_dec_detile_body: the four waves stream 4 KB of every plane per step
    const uint32_t t0 = (bx * (YK_Q_UNITS * 4) + wave) * 16 + (lane >> 2);
    uint32_t acc[4][4] = {};
    if ((bx + 1) * (uint32_t)YK_Q_TILES <= a.nTiles) {                        // every unit of the workgroup exists
#pragma unroll 1
        for (int g = 0; g < YK_Q_UNITS; g += KF) {                            // one trip for 8-bit sources; int32 planes: a unit's 16 B per sample at a time
            YkQUnit<CH, L> u[KF];
#pragma unroll
            for (int k = 0; k < KF; k++) yk_q_load<CH, L>(a, t0 + (g + k) * 64, rp, u[k]);
#pragma unroll
            for (int k = 0; k < KF; k++) {
                const uint32_t ts = yk_q_accumulate<CH, L>(u[k], acc);
                if (tileMap) yk_q_tile_store(tileMap, t0 + (g + k) * 64, rp, ts);
            }
        }
    } else {
        for (int k = 0; k < YK_Q_UNITS; k++) {                                // the last workgroup: tiles up to nTiles (a quad shares its tile)
            const uint32_t t = t0 + k * 64;
            if (t >= a.nTiles) continue;
            YkQUnit<CH, L> u;
            yk_q_load<CH, L>(a, t, rp, u);
            const uint32_t ts = yk_q_accumulate<CH, L>(u, acc);
            if (tileMap) yk_q_tile_store(tileMap, t, rp, ts);
        }
    }
    // wave: xor shuffles (every lane takes part: this point is reached by all 256 threads); waves: LDS
#pragma unroll
    for (int k = 0; k < CH; k++)
#pragma unroll
        for (int s = 0; s < 4; s++) {
            uint32_t v = acc[k][s];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64); v = s == 3 ? (o > v ? o : v) : v + o; }
            acc[k][s] = v;
        }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int s = 0; s < 4; s++) s_rec[wave][k * 4 + s] = k < CH ? acc[k][s] : 0u;
    }
    __syncthreads();
    if (threadIdx.x < YK_Q_REC) {
        const uint32_t i = threadIdx.x;
        uint32_t v = s_rec[0][i];
#pragma unroll
        for (int w = 1; w < YK_Q_THREADS / 64; w++) { const uint32_t o = s_rec[w][i]; v = (i & 3) == 3 ? (o > v ? o : v) : v + o; }
        a.partials[((size_t)f * gridDim.x + bx) * YK_Q_REC + i] = v;
    }
}

// one workgroup per frame: thread = (slice of the workgroups' records, entry of the record); sums and maxima in u64
__global__ __launch_bounds__(256) void yk_quality_fold_kernel(const uint32_t* __restrict__ partials, uint32_t nGroups, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_acc[256 / YK_Q_REC][YK_Q_REC];
    const uint32_t f = blockIdx.x, i = threadIdx.x & (YK_Q_REC - 1), slice = threadIdx.x / YK_Q_REC;
    const bool isMax = (i & 3) == 3;
    const uint32_t* p = partials + (size_t)f * nGroups * YK_Q_REC;
    unsigned long long v = 0;
    for (uint32_t g = slice; g < nGroups; g += 256 / YK_Q_REC) {
        const unsigned long long o = p[(size_t)g * YK_Q_REC + i];
        v = isMax ? (o > v ? o : v) : v + o;
    }
    s_acc[slice][i] = v;
    __syncthreads();
    if (threadIdx.x < YK_Q_REC) {
        v = s_acc[0][i];
        for (int s = 1; s < 256 / YK_Q_REC; s++) { const unsigned long long o = s_acc[s][i]; v = isMax ? (o > v ? o : v) : v + o; }
        out[(size_t)f * YK_Q_REC + i] = v;
    }
}

template <int CH, int L>
static void yk_q_launch(const YkQArgs& a, unsigned groups, unsigned nFrames, hipStream_t s) {
    hipLaunchKernelGGL((yk_quality_compare_kernel<CH, L>), dim3(groups, nFrames), dim3(YK_Q_THREADS), 0, s, a);
}

// The two launches and the one blocking read-back behind the yk_decode_compare_* entry points (yk_decode.hip validates and settles first).
// firstFrame / nFrames: the frames of the decode batch to compare; the source's frame 0 is compared with firstFrame.
int yk_quality_compare(yk_ctx* c, const YkQualitySrc& q, int firstFrame, int nFrames, int channels, yk_quality* out, uint32_t* devTileSse) {
    YkQArgs a = {};
    const size_t w = (size_t)c->dw, h = (size_t)c->dh, N = (size_t)nFrames;
    a.planes = yk_dec_frame(c, firstFrame).planes; a.planeSize = c->dPlaneSize; a.planesFrame = c->dStride.planes;
    if (channels == 4) {
        a.alphaFrame = c->dAlphaBatch ? c->dAlphaStride : 0;
        a.alpha = c->dAlpha + (size_t)firstFrame * a.alphaFrame; a.strideA = w;
    }
    a.src = q.src; a.rowBytes = q.rowBytes; a.planeBytes = q.planeBytes; a.srcFrame = q.frameStride;
    for (int k = 0; k < 4; k++) a.sp[k] = q.planes ? q.planes[k] : nullptr;
    a.strideElems = q.strideElems;
    a.tileW = (uint32_t)(w >> 3); a.nTiles = (uint32_t)(w >> 3) * (uint32_t)(h >> 3);
    const unsigned groups = (a.nTiles + YK_Q_TILES - 1) / YK_Q_TILES;
    // the handle's grow-only buffer: the folded u64 results of every frame, then the workgroups' records
    const size_t resBytes = N * YK_Q_REC * sizeof(unsigned long long), need = resBytes + N * groups * YK_Q_REC * sizeof(uint32_t);
    YK_HIP(c, c->qBuf.reserve(c->stream, need));
    unsigned long long* res = reinterpret_cast<unsigned long long*>(c->qBuf.p);
    a.partials = reinterpret_cast<uint32_t*>(c->qBuf + resBytes);
    a.tileMap = devTileSse;
    const int layout = q.planes ? YK_Q_PLANES : q.planeBytes ? YK_Q_CHW : q.srcChannels == 3 ? YK_Q_HWC3 : YK_Q_HWC4;
    { int rc = yk_stage_begin(c, YK_STAGE_DEC_COMPARE); if (rc) return rc; }
    const unsigned nf = (unsigned)nFrames;
    if (channels == 3) {
        if (layout == YK_Q_PLANES) yk_q_launch<3, YK_Q_PLANES>(a, groups, nf, c->stream);
        else if (layout == YK_Q_CHW) yk_q_launch<3, YK_Q_CHW>(a, groups, nf, c->stream);
        else if (layout == YK_Q_HWC3) yk_q_launch<3, YK_Q_HWC3>(a, groups, nf, c->stream);
        else yk_q_launch<3, YK_Q_HWC4>(a, groups, nf, c->stream);
    } else {
        if (layout == YK_Q_PLANES) yk_q_launch<4, YK_Q_PLANES>(a, groups, nf, c->stream);
        else if (layout == YK_Q_CHW) yk_q_launch<4, YK_Q_CHW>(a, groups, nf, c->stream);
        else yk_q_launch<4, YK_Q_HWC4>(a, groups, nf, c->stream);
    }
    YK_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(yk_quality_fold_kernel, dim3(nf), dim3(256), 0, c->stream, a.partials, groups, res);
    YK_HIP(c, hipGetLastError());
    { int rc = yk_stage_end(c, YK_STAGE_DEC_COMPARE); if (rc) return rc; }
    std::vector<unsigned long long> host(N * YK_Q_REC);
    YK_HIP(c, hipMemcpyAsync(host.data(), res, resBytes, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t f = 0; f < N; f++) {
        yk_quality r = {};
        for (int k = 0; k < channels; k++) {
            const unsigned long long* e = &host[f * YK_Q_REC + (size_t)k * 4];
            r.sse[k] = e[0]; r.sad[k] = e[1]; r.nDiff[k] = e[2]; r.maxAbs[k] = (uint32_t)e[3];
        }
        r.nSamples = (uint64_t)w * h;
        out[f] = r;
    }
    return YK_OK;
}
