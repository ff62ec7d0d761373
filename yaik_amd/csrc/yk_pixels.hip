// yk_pixels.hip — 8-bit interleaved RGB(A) pixels -> the handle's own int32 planes (yk_upload_pixels_u8 / yk_load_device_pixels_u8).
//
// The rule is Image::LoadPNG's widening loop (encoder/Image.cpp:211-221) with a row pitch: plane p at (x, y) = src[y * rowBytes + x * channels + p]
// for p < nPlanes (channels 4 with 3 planes drops the 4th byte).  ONE launch writes every plane of every frame (blockIdx.y = frame) into the
// layout yk_upload_planes fills: plane p of frame f at dst + f * frameElems + p * planeElems, rows of w int32.  Plain streaming: no LDS, no
// atomics; every source byte is read once and every int32 written once, (channels + 4 * nPlanes) bytes per pixel.
// A work unit is 4 pixels of one row (w is a multiple of 8, so rows hold whole units): one 12-byte (RGB) or 16-byte (RGBA) load and one int4
// store per plane.  Lane l of a wave takes unit base + l, so every load and store instruction of a wave covers one contiguous span (768 or
// 1024 bytes in, 1024 bytes out per plane).  A lane issues the loads of K units before its first store.
//   fast path (source base, rowBytes and frameBytes multiples of 16): the unit is read through a 16-byte (RGBA) or 4-byte (RGB) aligned
//     pointer.
//   byte path (any other base or pitch): the unit is read through a byte pointer, with no alignment assumed.  gfx950 allows unaligned global
//     loads, and hipcc merges those bytes into the same one dwordx3 / dwordx4 load per unit; what differs is only the alignment the code
//     claims.  DESIGN.md §11 has both paths' times.
// The host picks the path; it is uniform per launch.
#include "yk_common.h"

#define YK_PX_THREADS 256
#define YK_PX_K 4                   // units per lane in flight

typedef uint32_t yk_px4 __attribute__((ext_vector_type(4)));

struct YkPxArgs {
    const uint8_t* src; size_t rowBytes, frameBytes;
    int32_t* dst; size_t planeElems, frameElems;
    int w;
    uint32_t perRow;        // units per row (w / 4)
    uint32_t nUnits;        // rows * perRow
};

// 4 pixels of CH interleaved bytes, packed little-endian in wd[0..CH-1] -> one int4 store per plane
template <int CH, int NP>
__device__ __forceinline__ void yk_px_emit(const uint32_t* wd, int32_t* __restrict__ d, size_t planeElems) {
#pragma unroll
    for (int p = 0; p < NP; p++) {
        yk_px4 o;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int b = i * CH + p;
            o[i] = (wd[b >> 2] >> ((b & 3) * 8)) & 255u;
        }
        *reinterpret_cast<yk_px4*>(d + (size_t)p * planeElems) = o;
    }
}

template <int CH, bool FAST>
__device__ __forceinline__ void yk_px_load(const uint8_t* __restrict__ s, uint32_t* wd) {
    if constexpr (FAST && CH == 4) {
        const yk_px4 v = *reinterpret_cast<const yk_px4*>(s);
        wd[0] = v.x; wd[1] = v.y; wd[2] = v.z; wd[3] = v.w;
    } else if constexpr (FAST) {
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(s);
        wd[0] = s32[0]; wd[1] = s32[1]; wd[2] = s32[2];
    } else {
#pragma unroll
        for (int j = 0; j < CH; j++)
            wd[j] = (uint32_t)s[4 * j] | ((uint32_t)s[4 * j + 1] << 8) | ((uint32_t)s[4 * j + 2] << 16) | ((uint32_t)s[4 * j + 3] << 24);
    }
}

template <int CH, int NP, bool FAST>
__global__ __launch_bounds__(YK_PX_THREADS) void yk_unpack_u8_kernel(YkPxArgs a) {
    const uint8_t* __restrict__ src = a.src + (size_t)blockIdx.y * a.frameBytes;
    int32_t* __restrict__ dst = a.dst + (size_t)blockIdx.y * a.frameElems;
    const uint32_t u0 = blockIdx.x * (uint32_t)(YK_PX_THREADS * YK_PX_K) + threadIdx.x;
    if (u0 + (uint32_t)((YK_PX_K - 1) * YK_PX_THREADS) < a.nUnits) {
        // every unit of this lane exists: all loads first, then the stores
        uint32_t wd[YK_PX_K][CH];
        size_t dOff[YK_PX_K];
#pragma unroll
        for (int k = 0; k < YK_PX_K; k++) {
            const uint32_t u = u0 + (uint32_t)(k * YK_PX_THREADS), y = u / a.perRow, x0 = (u - y * a.perRow) * 4;
            yk_px_load<CH, FAST>(src + (size_t)y * a.rowBytes + (size_t)x0 * CH, wd[k]);
            dOff[k] = (size_t)y * a.w + x0;
        }
#pragma unroll
        for (int k = 0; k < YK_PX_K; k++) yk_px_emit<CH, NP>(wd[k], dst + dOff[k], a.planeElems);
        return;
    }
    for (int k = 0; k < YK_PX_K; k++) {                                       // the last units of the frame
        const uint32_t u = u0 + (uint32_t)(k * YK_PX_THREADS);
        if (u >= a.nUnits) return;
        const uint32_t y = u / a.perRow, x0 = (u - y * a.perRow) * 4;
        uint32_t wd[CH];
        yk_px_load<CH, FAST>(src + (size_t)y * a.rowBytes + (size_t)x0 * CH, wd);
        yk_px_emit<CH, NP>(wd, dst + (size_t)y * a.w + x0, a.planeElems);
    }
}

template <int CH, int NP, bool FAST>
static void yk_px_launch(const YkPxArgs& a, int nFrames, hipStream_t s) {
    const uint32_t perBlock = YK_PX_THREADS * YK_PX_K;
    hipLaunchKernelGGL((yk_unpack_u8_kernel<CH, NP, FAST>), dim3((a.nUnits + perBlock - 1) / perBlock, nFrames), dim3(YK_PX_THREADS), 0, s, a);
}

// rows (per frame) x w pixels of `channels` bytes at src (+ f * frameBytes for frame f) -> c->nPlanes planes at dst; timed as YK_STAGE_UNPACK
int yk_launch_unpack_u8(yk_ctx* c, const uint8_t* src, size_t rowBytes, size_t frameBytes, int channels, int rows, int nFrames,
                        int32_t* dst, size_t planeElems, size_t frameElems) {
    const bool fast = ((uintptr_t)src & 15) == 0 && (rowBytes & 15) == 0 && (nFrames == 1 || (frameBytes & 15) == 0);
    YkPxArgs a;
    a.src = src; a.rowBytes = rowBytes; a.frameBytes = nFrames > 1 ? frameBytes : 0;
    a.dst = dst; a.planeElems = planeElems; a.frameElems = nFrames > 1 ? frameElems : 0;
    a.w = c->fullW;
    a.perRow = (uint32_t)(c->fullW / 4);
    a.nUnits = (uint32_t)rows * a.perRow;
    { int rc = yk_stage_begin(c, YK_STAGE_UNPACK); if (rc) return rc; }
    if (channels == 4 && c->nPlanes == 4) { if (fast) yk_px_launch<4, 4, true>(a, nFrames, c->stream); else yk_px_launch<4, 4, false>(a, nFrames, c->stream); }
    else if (channels == 4)               { if (fast) yk_px_launch<4, 3, true>(a, nFrames, c->stream); else yk_px_launch<4, 3, false>(a, nFrames, c->stream); }
    else                                  { if (fast) yk_px_launch<3, 3, true>(a, nFrames, c->stream); else yk_px_launch<3, 3, false>(a, nFrames, c->stream); }
    YK_HIP(c, hipGetLastError());
    { int rc = yk_stage_end(c, YK_STAGE_UNPACK); if (rc) return rc; }
    return YK_OK;
}
