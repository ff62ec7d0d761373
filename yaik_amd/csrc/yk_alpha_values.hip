// 'ALPM' alpha value chunk on the device.
//   yk_alpha_values   EncoderContext::ProcessAlpha (encoder/EncoderContext.cpp:1429-1682, make1BitStream :317-355): box, class, payload
//                     (8-bit, 1-bit, and the 6-bit mask mode of force8Bit = false)
//   yk_alpha_values_batch   the same for every frame of the handle.  There is one encode path: yk_ave_classify (box, slots, class) and
//                     yk_ave_chunk (class -> mode, box, bytes) serve both entry points, the single image is a batch of one that copies its
//                     payload out and, for force8Bit = false, packs the 6-bit payload from its slot
//   yk_alpha_values_mask_batch   ProcessAlpha(force8Bit[f]) per frame: the same path, and batch forms of the three 6-bit kernels over the analog
//                     frames whose force8Bit is 0, each into a 6-bit slot of its own
//   yk_decode_alpha   Decompress1BitMaskAlign8NoMask (decoder/YAIK_Alpha.cpp:25-112), Decompress6BitTo8BitAlphaNoMask (:114-235),
//                     Decompress6BitTo8BitAlphaUsingMipmapMask (:237-376), Decompress8BitTo8BitAlphaNoMask (:377-444): the full w x h plane
//                     in HBM (0 outside the box), kept for yk_decode_output_alpha.
//   yk_decode_alpha_[mask_]batch_device   the same planes for every frame of a decode batch; the mask modes read the 'MIPM' tile bitmap in place
//                     (their two loops are written once, over the source of the mask bit)
#include "yk_common.h"
#include <climits>

namespace {

__device__ __forceinline__ uint8_t yk_av_expand6(uint32_t v6, bool inv) {
    const uint32_t x = inv ? 63u - v6 : v6;
    return (uint8_t)((x << 2) | (x >> 4));
}
// sample k of a 4-values-in-3-bytes stream (EncoderContext.cpp:1528-1541); bytes at or beyond n read as 0
__device__ __forceinline__ uint32_t yk_av_sample6(const uint8_t* __restrict__ s, size_t n, size_t k) {
    const size_t g = (k >> 2) * 3;
    const uint32_t b0 = g < n ? s[g] : 0u, b1 = g + 1 < n ? s[g + 1] : 0u, b2 = g + 2 < n ? s[g + 2] : 0u;
    switch (k & 3) {
    case 0: return b0 & 63u;
    case 1: return (b0 >> 6) | ((b1 & 15u) << 2);
    case 2: return (b1 >> 4) | ((b2 & 3u) << 4);
    default: return b2 >> 2;
    }
}

// modes 1 (1 bit), 4 / 5 (6 bit, no mask), 6 (8 bit): the value of plane pixel i (flat index); every pixel of the plane is written.
// refQuirk (mode 1 only): the reference's row loop `while (--cnt)` (YAIK_Alpha.cpp:76) decodes w/8 - 1 bytes per row and then skips
// w - bw pixels, so every row lands 8 pixels left of the previous one; pixels it never writes are 0.
__device__ __forceinline__ uint8_t yk_av_pixel(size_t i, int x, int y, const uint8_t* __restrict__ pay, size_t n, int mode, int refQuirk, int bx,
                                               int by, int bw, int bh, int W) {
    uint8_t v = 0;
    if (mode == 1 && refQuirk) {
        const long long rel = (long long)i - ((long long)by * W + bx);
        const int blk = bw >> 3;
        if (rel >= 0 && W > 8) {                                                // W = 8: a row holds w/8 - 1 = 0 bytes
            const long long r = rel / (W - 8), o = rel % (W - 8);
            if (r < bh && o < 8ll * (blk - 1)) {
                const size_t byte = (size_t)r * (blk - 1) + (size_t)(o >> 3);
                v = (byte < n && ((pay[byte] >> (o & 7)) & 1)) ? 255 : 0;
            }
        }
    } else {
        const int c = x - bx, r = y - by;
        if (c >= 0 && c < bw && r >= 0 && r < bh) {
            if (mode == 6) {
                const size_t k = (size_t)r * bw + c;
                v = k < n ? pay[k] : 0;
            } else if (mode == 1) {
                const size_t byte = (size_t)r * (bw >> 3) + (c >> 3);
                v = (byte < n && ((pay[byte] >> (c & 7)) & 1)) ? 255 : 0;
            } else {
                const size_t k = (size_t)r * bw + c;      // bw is a multiple of 4: the rows are whole 3-byte groups
                v = yk_av_expand6(yk_av_sample6(pay, n, k), mode == 5);
            }
        }
    }
    return v;
}
// one thread = 16 consecutive pixels of the flat plane and one 16-byte store (the plane is w * h bytes, a multiple of 64).  W a multiple of 16:
// the 16 pixels lie in one row.  RAGGED (W = 8 mod 16): each half of 8 pixels lies in one row, the second half may start the next row
template <bool RAGGED>
__device__ __forceinline__ void yk_av_decode_body(const uint8_t* __restrict__ pay, size_t n, int mode, int refQuirk, int bx, int by, int bw, int bh, int W, int H,
                                                  uint8_t* __restrict__ out, uint32_t blk) {
    const size_t i0 = ((size_t)blk * 256 + threadIdx.x) * 16;
    if (i0 >= (size_t)W * H) return;
    uint32_t word[4];
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        if (!RAGGED && hf) break;
        const size_t ih = i0 + (RAGGED ? 8 * hf : 0);
        const int y = (int)((uint32_t)ih / (uint32_t)W), x0 = (int)(ih - (size_t)y * W);   // one 32-bit divide per row piece (w * h < 2^31)
#pragma unroll
        for (int q = (RAGGED ? 2 * hf : 0); q < (RAGGED ? 2 * hf + 2 : 4); q++) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                v |= (uint32_t)yk_av_pixel(i0 + q * 4 + k, x0 + (int)(i0 + q * 4 + k - ih), y, pay, n, mode, refQuirk, bx, by, bw, bh, W) << (8 * k);
            word[q] = v;
        }
    }
    *reinterpret_cast<uint4*>(out + i0) = make_uint4(word[0], word[1], word[2], word[3]);
}
template <bool RAGGED>
__global__ __launch_bounds__(256) void yk_av_decode_kernel(const uint8_t* __restrict__ pay, size_t n, int mode, int refQuirk, int bx, int by, int bw, int bh,
                                                           int W, int H, uint8_t* __restrict__ out) {
    yk_av_decode_body<RAGGED>(pay, n, mode, refQuirk, bx, by, bw, bh, W, H, out, blockIdx.x);
}
// a batch (yk_decode_alpha_batch_device): frame blockIdx.y's record is read through uniform loads, its plane is at out + f * planeStride.  A
// frame without a chunk (mode -1) gets the constant `fill` (the byte in all four lanes of a dword), still one 16-byte store per thread
struct YkAvDecFrame { const uint8_t* pay; unsigned long long n; int32_t mode, bx, by, bw, bh, pad[3]; };
template <bool RAGGED>
__global__ __launch_bounds__(256) void yk_av_decode_batch_kernel(const YkAvDecFrame* __restrict__ tab, int W, int H, uint8_t* __restrict__ out, size_t planeStride,
                                                                 uint32_t fill) {
    const YkAvDecFrame r = tab[blockIdx.y];
    out += (size_t)blockIdx.y * planeStride;
    if (r.mode < 0) {
        const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
        if (i0 < (size_t)W * H) *reinterpret_cast<uint4*>(out + i0) = make_uint4(fill, fill, fill, fill);
        return;
    }
    yk_av_decode_body<RAGGED>(r.pay, (size_t)r.n, r.mode, 0, r.bx, r.by, r.bw, r.bh, W, H, out, blockIdx.x);
}

// mask modes 2 / 3.  The row-count and the decode loop are written once, over a bit source `m` that answers "is box pixel (r, c) selected"
// through yk_av_selected: YkAvMaskBits (the decoded mask buffer of yk_decode_alpha) or YkAvMaskFrame (a batch frame's 'MIPM' tile bitmap).
// YkAvMaskBits: the bit of box pixel (c, r) in the decoder's mipMapMask (read linearly with stride maskBBox.w from the alpha box's
// origin, in 32-bit arithmetic like the reference's u32 mipmapPos); bits outside the mask buffer read 0
struct YkAvMaskBits { const uint8_t* mask; size_t maskBytes; uint32_t base, stride; };
__device__ __forceinline__ bool yk_av_maskbit(const uint8_t* __restrict__ mask, size_t maskBytes, uint32_t base, uint32_t stride, int r, int c) {
    const uint32_t pos = base + stride * (uint32_t)r + (uint32_t)c;
    return (size_t)(pos >> 3) < maskBytes && ((mask[pos >> 3] >> (pos & 7)) & 1);
}
__device__ __forceinline__ bool yk_av_selected(const YkAvMaskBits& m, int r, int c) { return yk_av_maskbit(m.mask, m.maskBytes, m.base, m.stride, r, c); }
// One record per masked frame of a batch (yk_decode_alpha_mask_batch_device), read through uniform loads.  The mask bit is derived straight from
// the frame's 'MIPM' tile bitmap (1 bit per 16x16 tile, LSB first, read in place): yk_dec_mask_kernel writes tile (tx, ty) of a tbw x tbh box as
// the four u64 words ty * 4 * tbw + {2 tx, 2 tx + 1, 2 tbw + 2 tx, 2 tbw + 2 tx + 1}, all ones or all zeros, so bit `pos` of that buffer is the
// tile bit of word q = pos >> 6.  nq = 4 * tbw * tbh words = the maskBytes = tbw * tbh * 32 of the single-image call: bits at or beyond read 0.
struct YkAvMaskFrame {
    const uint8_t* pay; unsigned long long n; const uint8_t* bits;
    uint32_t base, stride, tbw, nq;          // base / stride as in YkAvMaskBits (stride = tbw * 16)
    int32_t bx, by, bw, bh, inv, frame;
    uint32_t oRows, pad;                     // rowCnt[bh], rowStart[bh + 1] at rows + oRows
};
__device__ __forceinline__ bool yk_av_tilebit(const YkAvMaskFrame& m, int r, int c) {
    const uint32_t pos = m.base + m.stride * (uint32_t)r + (uint32_t)c, q = pos >> 6;
    if (q >= m.nq) return false;
    const uint32_t per = 4u * m.tbw, i = (q / per) * m.tbw + (((q % per) % (2u * m.tbw)) >> 1);
    return (m.bits[i >> 3] >> (i & 7)) & 1;
}
__device__ __forceinline__ bool yk_av_selected(const YkAvMaskFrame& m, int r, int c) { return yk_av_tilebit(m, r, c); }
// one wave per box row: count of mask-selected pixels
template <class BITS>
__device__ __forceinline__ void yk_av_rowcount_body(const BITS& m, int r, int bw, uint32_t* __restrict__ rowCnt) {
    uint32_t cnt = 0;
    for (int c = threadIdx.x; c < bw; c += 64) cnt += yk_av_selected(m, r, c) ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if (threadIdx.x == 0) rowCnt[r] = cnt;
}
// one wave per box row: sample index of a selected pixel = the row's start k + selected pixels to its left (ballot + popcount); the state of the
// reference's 4-value cycle is that index, it carries across rows like `state` does (YAIK_Alpha.cpp:313).  `row` = the box row in the plane
template <class BITS>
__device__ __forceinline__ void yk_av_maskdecode_body(const BITS& m, int r, int bw, const uint8_t* __restrict__ pay, size_t n, bool inv, uint32_t k,
                                                      uint8_t* __restrict__ row) {
    const int lane = threadIdx.x;
    for (int c0 = 0; c0 < bw; c0 += 64) {
        const int c = c0 + lane;
        const bool sel = c < bw && yk_av_selected(m, r, c);
        const unsigned long long b = __ballot(sel);
        const uint32_t before = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (c < bw) row[c] = sel ? yk_av_expand6(yk_av_sample6(pay, n, (size_t)k + before), inv) : 0;
        k += (uint32_t)__popcll(b);
    }
}
__global__ __launch_bounds__(64) void yk_av_rowcount_kernel(const uint8_t* __restrict__ mask, size_t maskBytes, uint32_t base, uint32_t stride, int bw,
                                                            uint32_t* __restrict__ rowCnt) {
    yk_av_rowcount_body(YkAvMaskBits{ mask, maskBytes, base, stride }, (int)blockIdx.x, bw, rowCnt);
}
// one workgroup: exclusive prefix of the row counts, total in rowStart[bh].  Thread t owns a run of ceil(bh / 1024) rows; the run sums are
// scanned in LDS.  Returns thread t's inclusive sum: thread 1023 holds the total
__device__ __forceinline__ uint32_t yk_av_rowscan_body(const uint32_t* __restrict__ rowCnt, int bh, uint32_t* __restrict__ rowStart, uint32_t* s) {
    const int t = threadIdx.x, per = (bh + 1023) / 1024, r0 = t * per, r1 = min(r0 + per, bh);
    uint32_t sum = 0;
    for (int r = r0; r < r1; r++) sum += rowCnt[r];
    s[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = t >= o ? s[t - o] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    uint32_t run = s[t] - sum;
    for (int r = r0; r < r1; r++) { rowStart[r] = run; run += rowCnt[r]; }
    if (t == 1023) rowStart[bh] = s[1023];
    return s[t];
}
__global__ __launch_bounds__(1024) void yk_av_rowscan_kernel(const uint32_t* __restrict__ rowCnt, int bh, uint32_t* __restrict__ rowStart) {
    __shared__ uint32_t s[1024];
    (void)yk_av_rowscan_body(rowCnt, bh, rowStart, s);
}
__global__ __launch_bounds__(64) void yk_av_maskdecode_kernel(const uint8_t* __restrict__ pay, size_t n, const uint8_t* __restrict__ mask, size_t maskBytes,
                                                              uint32_t base, uint32_t stride, int bx, int by, int bw, int inv,
                                                              const uint32_t* __restrict__ rowStart, int W, uint8_t* __restrict__ out) {
    const int r = blockIdx.x;
    yk_av_maskdecode_body(YkAvMaskBits{ mask, maskBytes, base, stride }, r, bw, pay, n, inv != 0, rowStart[r], out + (size_t)(by + r) * W + bx);
}
// the same three in a batch: masked frame blockIdx.y's record (the grids are sized from the tallest box: waves below this frame's box leave at once)
__global__ __launch_bounds__(64) void yk_av_rowcount_batch_kernel(const YkAvMaskFrame* __restrict__ tab, uint32_t* __restrict__ rows) {
    const YkAvMaskFrame m = tab[blockIdx.y];
    if ((int)blockIdx.x < m.bh) yk_av_rowcount_body(m, (int)blockIdx.x, m.bw, rows + m.oRows);
}
// one workgroup per masked frame: yk_av_rowscan_kernel's scan, and the frame's status word: 1 when the payload is shorter than the mask selects
__global__ __launch_bounds__(1024) void yk_av_rowscan_batch_kernel(const YkAvMaskFrame* __restrict__ tab, uint32_t* __restrict__ rows,
                                                                   int32_t* __restrict__ status) {
    __shared__ uint32_t s[1024];
    const YkAvMaskFrame m = tab[blockIdx.x];
    const uint32_t total = yk_av_rowscan_body(rows + m.oRows, m.bh, rows + m.oRows + m.bh, s);
    if (threadIdx.x == 1023) status[blockIdx.x] = ((unsigned long long)total * 6 + 7) / 8 > m.n ? 1 : 0;
}
// the plane was zeroed by the unmasked launch in front
__global__ __launch_bounds__(64) void yk_av_maskdecode_batch_kernel(const YkAvMaskFrame* __restrict__ tab, const uint32_t* __restrict__ rows, int W,
                                                                    uint8_t* __restrict__ out, size_t planeStride) {
    const YkAvMaskFrame m = tab[blockIdx.y];
    const int r = blockIdx.x;
    if (r >= m.bh) return;
    yk_av_maskdecode_body(m, r, m.bw, m.pay, (size_t)m.n, m.inv != 0, rows[m.oRows + m.bh + r],
                          out + (size_t)m.frame * planeStride + (size_t)(m.by + r) * W + m.bx);
}

// ---- encode: EncoderContext::ProcessAlpha (encoder/EncoderContext.cpp:1429-1682) --------------------------------------------------
// One set of kernels for yk_alpha_values (one frame) and yk_alpha_values_batch (N): blockIdx.z = frame (box) or record (class, pack1), frame f's
// plane at alpha + f * frameElems (frameElems = 0 with one frame), its bounds 16 ints, its state 8 ints:
// st[0..3] = bL, bT, bR, bB of the samples with v >> 2 != 0 (min / min / max / max, inclusive); st[4] = "a sample in 1..254 in the rounded box",
// st[5] = "a sample != 255 in the rounded box".
#define YK_AV_ROWS 16
// 4 samples at p: one 16-byte load when the plane's rows are 16-byte aligned (VEC), 4 loads otherwise
template <bool VEC>
__device__ __forceinline__ int4 yk_ave_load4(const int32_t* __restrict__ p) {
    if (VEC) return *reinterpret_cast<const int4*>(p);
    return make_int4(p[0], p[1], p[2], p[3]);
}
// box of v >> 2 != 0 inside the MipPrefilter bounds (read on the device from the alpha stage's result); one thread = 4 pixels of YK_AV_ROWS rows
template <bool VEC>
__global__ __launch_bounds__(256) void yk_ave_box_batch_kernel(const int32_t* __restrict__ alpha, unsigned long long frameElems, int stride,
                                                               const int32_t* __restrict__ bounds, int W, int H, int32_t* __restrict__ st) {
    const size_t f = blockIdx.z;
    alpha += f * frameElems; bounds += f * 16; st += f * 8;
    // the region starts on a multiple of 16 (kept 16x16 tiles); the loads start on the multiple of 4 at or below it whatever it is
    const int xs = max(bounds[0], 0), x0 = xs & ~3, y0 = max(bounds[1], 0), x1 = min(bounds[2], W), y1 = min(bounds[3], H);
    const int x = x0 + ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4, yb = y0 + (int)blockIdx.y * YK_AV_ROWS;
    int mnx = INT_MAX, mny = INT_MAX, mxx = -1, mxy = -1;
    if (x < x1)
        for (int y = yb; y < min(yb + YK_AV_ROWS, y1); y++) {
            const int4 q = yk_ave_load4<VEC>(alpha + (size_t)y * stride + x);            // x < x1 <= W, W a multiple of 16: all 4 in the row
            const int v[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (x + k >= xs && x + k < x1 && (v[k] >> 2) != 0) { mnx = min(mnx, x + k); mxx = max(mxx, x + k); mny = min(mny, y); mxy = max(mxy, y); }
        }
    for (int o = 32; o > 0; o >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, o, 64)); mny = min(mny, __shfl_xor(mny, o, 64));
        mxx = max(mxx, __shfl_xor(mxx, o, 64)); mxy = max(mxy, __shfl_xor(mxy, o, 64));
    }
    // one lane per wave, and only the atomics that can still change the box: thousands of waves on four words would serialise in L2
    // (a stale read only costs an unneeded atomic)
    if ((threadIdx.x & 63) == 0 && mxx >= 0) {
        const volatile int32_t* v = st;
        if (mnx < v[0]) atomicMin(&st[0], mnx);
        if (mny < v[1]) atomicMin(&st[1], mny);
        if (mxx > v[2]) atomicMax(&st[2], mxx);
        if (mxy > v[3]) atomicMax(&st[3], mxy);
    }
}
// one record per frame that has a box (the box rounded to 4 in x, the frame, the offset of its payload slot); record blockIdx.z is read through
// uniform loads.  The grids are sized from the largest box: workgroups outside this frame's box leave at once.
struct YkAvFrame { int32_t bL, bT, bw, bh; unsigned long long off; int32_t frame, pad; };
// the three class flags over the box rounded to 4 in x (isAnalogAlpha, isAll1; isAll0 is false once the box is not empty) and, in the same
// read, the 8-bit payload (every sample of the box, row-major, in the frame's slot): one thread = 4 pixels = one 4-byte store
template <bool VEC>
__global__ __launch_bounds__(256) void yk_ave_class_batch_kernel(const int32_t* __restrict__ alpha, unsigned long long frameElems, int stride,
                                                                 const YkAvFrame* __restrict__ tab, uint8_t* __restrict__ pay, int32_t* __restrict__ st) {
    const YkAvFrame f = tab[blockIdx.z];
    if ((int)blockIdx.y >= f.bh || (int)blockIdx.x * 1024 >= f.bw) return;
    alpha += (size_t)f.frame * frameElems; pay += f.off; st += (size_t)f.frame * 8;
    const int r = blockIdx.y, c = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    bool analog = false, not255 = false;
    if (c < f.bw) {
        const int4 q = yk_ave_load4<VEC>(alpha + (size_t)(f.bT + r) * stride + f.bL + c);   // bL and c are multiples of 4
        const int vs[4] = { q.x, q.y, q.z, q.w };
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int v = vs[k];
            analog |= v > 0 && v < 255; not255 |= v != 255;
            word |= (uint32_t)(v & 255) << (8 * k);
        }
        *reinterpret_cast<uint32_t*>(pay + (size_t)r * f.bw + c) = word;    // off, bw and c are multiples of 4
    }
    const unsigned long long a = __ballot(analog), n = __ballot(not255);
    if ((threadIdx.x & 63) == 0) {                                         // a flag is set once: later waves only read it
        const volatile int32_t* v = st;
        if (a && !v[4]) atomicOr(&st[4], 1);
        if (n && !v[5]) atomicOr(&st[5], 1);
    }
}
// make1BitStream (:317-355) for the frames the class kernel found binary (flags: not analog, not all 255), on the box re-aligned to 8 as
// yk_ave_chunk does it on the host: bit (v & 1) of every sample, LSB first; one thread = one output byte.  The 1-bit payload replaces the
// 8-bit one in the frame's slot (it is never longer)
__global__ __launch_bounds__(256) void yk_ave_pack1_batch_kernel(const int32_t* __restrict__ alpha, unsigned long long frameElems, int stride,
                                                                 const YkAvFrame* __restrict__ tab, uint8_t* __restrict__ pay, const int32_t* __restrict__ st) {
    const YkAvFrame f = tab[blockIdx.z];
    const int32_t* s = st + (size_t)f.frame * 8;
    if (s[4] != 0 || s[5] == 0) return;
    const int bL = (f.bL >> 3) << 3, bR = ((f.bL + f.bw + 7) >> 3) << 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, perRow = (size_t)((bR - bL) >> 3);
    if (i >= perRow * f.bh) return;
    const int r = (int)(i / perRow), c = (int)(i % perRow) * 8;
    const int32_t* p = alpha + (size_t)f.frame * frameElems + (size_t)(f.bT + r) * stride + bL + c;
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) b |= (uint32_t)(p[k] & 1) << k;
    pay[f.off + i] = (uint8_t)b;
}

// ---- force8Bit = false: IS_6_BIT_USEMIPMAPMASK_INVERSE (:1503-1565) -----------------------------------------------------------------------
// The selected set is the reference's per-pixel mipmapMask as MipPrefilter leaves it: every pixel of a kept 16x16 tile, or every pixel when
// the kept tiles span the image (no 'MIPM' chunk, the mask is set again to 255 at :1401).  So a box row's selected pixels are whole runs of
// tile columns, the same for the 16 rows of a tile band, and a sample's output index follows from the keep flags alone.  bL, bR and the tile
// edges are multiples of 4: every run is whole 4-sample groups, and a group of the box is one 3-byte group of the payload.
__device__ __forceinline__ bool yk_ave_all_kept(const int32_t* __restrict__ b, int W, int H) { return b[0] == 0 && b[1] == 0 && b[2] == W && b[3] == H; }
// one wave per tile band of the box: colPre[band][i] = selected samples of one band row left of tile column txB + i, bandS = per row,
// bandCnt = per band (bandS x the band's rows in the box)
__device__ __forceinline__ void yk_ave_band_body(const uint8_t* __restrict__ keep, int mtW, int mtH, const int32_t* __restrict__ bounds, int W, int H,
                                                 int bL, int bT, int bR, int bB, int ncol, uint32_t* __restrict__ colPre, uint32_t* __restrict__ bandS,
                                                 uint32_t* __restrict__ bandCnt) {
    const int b = blockIdx.x, lane = threadIdx.x, ty = (bT >> 4) + b, txB = bL >> 4;
    const bool all = yk_ave_all_kept(bounds, W, H);
    uint32_t carry = 0;
    for (int i0 = 0; i0 < ncol; i0 += 64) {
        const int i = i0 + lane, tx = txB + i;
        uint32_t v = 0;
        if (i < ncol && tx < mtW && ty < mtH && (all || keep[(size_t)ty * mtW + tx])) v = (uint32_t)(min(bR, tx * 16 + 16) - max(bL, tx * 16));
        uint32_t s = v;                                                    // inclusive scan over the wave
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(s, o, 64); if (lane >= o) s += t; }
        if (i < ncol) colPre[(size_t)b * ncol + i] = carry + s - v;
        carry += __shfl(s, 63, 64);
    }
    if (lane == 0) {
        bandS[b] = carry;
        bandCnt[b] = carry * (uint32_t)(min(bB, ty * 16 + 16) - max(bT, ty * 16));
    }
}
__global__ __launch_bounds__(64) void yk_ave_band_kernel(const uint8_t* __restrict__ keep, int mtW, int mtH, const int32_t* __restrict__ bounds, int W, int H,
                                                         int bL, int bT, int bR, int bB, int ncol, uint32_t* __restrict__ colPre, uint32_t* __restrict__ bandS,
                                                         uint32_t* __restrict__ bandCnt) {
    yk_ave_band_body(keep, mtW, mtH, bounds, W, H, bL, bT, bR, bB, ncol, colPre, bandS, bandCnt);
}
// one thread = one 4-sample group of the u8 box the class kernel wrote (one 4-byte load) = one 3-byte group of the payload when its tile is
// selected: index = band start + rows of the band above it x bandS + colPre + its offset in the tile's run; values 63 - (v >> 2), LSB first
__device__ __forceinline__ void yk_ave_pack6_body(const uint8_t* __restrict__ box, int bL, int bT, int bw, int bh, const uint8_t* __restrict__ keep,
                                                  int mtW, int mtH, const int32_t* __restrict__ bounds, int W, int H, int ncol, int nb,
                                                  const uint32_t* __restrict__ colPre, const uint32_t* __restrict__ bandS,
                                                  const uint32_t* __restrict__ bandStart, uint8_t* __restrict__ out, size_t cap) {
    const int c = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4, r = blockIdx.y;
    if (c >= bw || r >= bh) return;
    const int x = bL + c, y = bT + r, tx = x >> 4, ty = y >> 4;
    if (tx >= mtW || ty >= mtH) return;
    if (!yk_ave_all_kept(bounds, W, H) && !keep[(size_t)ty * mtW + tx]) return;
    const int b = ty - (bT >> 4), i = tx - (bL >> 4);
    if (b < 0 || b >= nb || i < 0 || i >= ncol) return;
    const uint32_t k = bandStart[b] + (uint32_t)(y - max(bT, ty * 16)) * bandS[b] + colPre[(size_t)b * ncol + i] + (uint32_t)(x - max(bL, tx * 16));
    const size_t o = (size_t)(k >> 2) * 3;                                 // k is a multiple of 4
    if (o + 3 > cap) return;
    const uint32_t w = *reinterpret_cast<const uint32_t*>(box + (size_t)r * bw + c);   // bw and c are multiples of 4
    const uint32_t q0 = 63u - ((w >> 2) & 63u), q1 = 63u - ((w >> 10) & 63u), q2 = 63u - ((w >> 18) & 63u), q3 = 63u - (w >> 26);
    out[o] = (uint8_t)(q0 | (q1 << 6));
    out[o + 1] = (uint8_t)((q1 >> 2) | (q2 << 4));
    out[o + 2] = (uint8_t)((q2 >> 4) | (q3 << 2));
}
__global__ __launch_bounds__(256) void yk_ave_pack6_kernel(const uint8_t* __restrict__ box, int bL, int bT, int bw, int bh, const uint8_t* __restrict__ keep,
                                                           int mtW, int mtH, const int32_t* __restrict__ bounds, int W, int H, int ncol, int nb,
                                                           const uint32_t* __restrict__ colPre, const uint32_t* __restrict__ bandS,
                                                           const uint32_t* __restrict__ bandStart, uint8_t* __restrict__ out, size_t cap) {
    yk_ave_pack6_body(box, bL, bT, bw, bh, keep, mtW, mtH, bounds, W, H, ncol, nb, colPre, bandS, bandStart, out, cap);
}
// the same three in a batch (yk_alpha_values_mask_batch): one record per frame classed analog whose force8Bit is 0, record blockIdx.z read through
// uniform loads.  keep / bounds = the frame's keep flags and image-wide box, box = its u8 slot in avPay, out = its 6-bit slot of `cap` bytes;
// its prefixes lie in one u32 arena at `arena`: colPre[nb * ncol], bandS[nb], bandCnt[nb], bandStart[nb + 1].  The grids are sized from the
// largest record: workgroups outside their frame's box leave at once.
struct YkAv6Rec {
    const uint8_t* keep; const int32_t* bounds; const uint8_t* box; uint8_t* out;
    unsigned long long cap, arena;
    int32_t bL, bT, bR, bB, ncol, nb;
};
__global__ __launch_bounds__(64) void yk_ave_band_batch_kernel(const YkAv6Rec* __restrict__ tab, int mtW, int mtH, int W, int H, uint32_t* __restrict__ u32s) {
    const YkAv6Rec r = tab[blockIdx.z];
    if ((int)blockIdx.x >= r.nb) return;
    uint32_t* colPre = u32s + r.arena;
    uint32_t* bandS = colPre + (size_t)r.nb * r.ncol;
    yk_ave_band_body(r.keep, mtW, mtH, r.bounds, W, H, r.bL, r.bT, r.bR, r.bB, r.ncol, colPre, bandS, bandS + r.nb);
}
// one wave per record: exclusive prefix of its bandCnt with the carry across the 64-band steps, the total in bandStart[nb] and in totals[record]
// (one contiguous array: the selected counts of every record come back in one copy)
__global__ __launch_bounds__(64) void yk_ave_bandscan_batch_kernel(const YkAv6Rec* __restrict__ tab, uint32_t* __restrict__ u32s, uint32_t* __restrict__ totals) {
    const YkAv6Rec r = tab[blockIdx.z];
    const int lane = threadIdx.x;
    const uint32_t* bandCnt = u32s + r.arena + (size_t)r.nb * r.ncol + r.nb;
    uint32_t* bandStart = u32s + r.arena + (size_t)r.nb * r.ncol + 2 * (size_t)r.nb;
    uint32_t carry = 0;
    for (int i0 = 0; i0 < r.nb; i0 += 64) {
        const int i = i0 + lane;
        const uint32_t v = i < r.nb ? bandCnt[i] : 0u;
        uint32_t s = v;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(s, o, 64); if (lane >= o) s += t; }
        if (i < r.nb) bandStart[i] = carry + s - v;
        carry += __shfl(s, 63, 64);
    }
    if (lane == 0) { bandStart[r.nb] = carry; totals[blockIdx.z] = carry; }
}
__global__ __launch_bounds__(256) void yk_ave_pack6_batch_kernel(const YkAv6Rec* __restrict__ tab, int mtW, int mtH, int W, int H, const uint32_t* __restrict__ u32s) {
    const YkAv6Rec r = tab[blockIdx.z];
    const int bw = r.bR - r.bL, bh = r.bB - r.bT;
    if ((int)blockIdx.y >= bh || (int)blockIdx.x * 1024 >= bw) return;
    const uint32_t* colPre = u32s + r.arena;
    const uint32_t* bandS = colPre + (size_t)r.nb * r.ncol;
    yk_ave_pack6_body(r.box, r.bL, r.bT, bw, bh, r.keep, mtW, mtH, r.bounds, W, H, r.ncol, r.nb, colPre, bandS, bandS + 2 * (size_t)r.nb, r.out, (size_t)r.cap);
}

}  // namespace

extern "C" {

int yk_decode_alpha(yk_ctx* c, int mode, const int32_t bbox[4], const uint8_t* payload, size_t n, const uint8_t* mask, size_t maskBytes,
                    const int32_t maskBBox[4], int refQuirk) {
    if (!c || !bbox || (!payload && n)) return YK_ERR_BAD_ARG;
    YK_DEC_NO_BATCH(c, "yk_decode_alpha");
    if (!yk_dec_begun(c)) return yk_fail(c, YK_ERR_STATE, "yk_decode_begin first");
    const int W = c->dw, H = c->dh;
    const int bx = bbox[0], by = bbox[1], bw = bbox[2], bh = bbox[3];
    // CheckInBound2D (YAIK_Alpha.cpp:12-23) read as "in bounds passes" (it has no `return true`), for every mode; an empty box is refused
    if (bx < 0 || by < 0 || bw <= 0 || bh <= 0 || bx >= W || by >= H || bx + bw > W || by + bh > H) return yk_fail(c, YK_ERR_BAD_ARG, "alpha box outside the image");
    size_t need = 0;
    switch (mode) {
    case 1: if (bw & 7) return yk_fail(c, YK_ERR_BAD_ARG, "1-bit alpha box width not a multiple of 8");
            need = (size_t)bh * ((bw >> 3) - (refQuirk ? 1 : 0)); break;
    case 4: case 5: if (bw & 3) return yk_fail(c, YK_ERR_BAD_ARG, "6-bit alpha box width not a multiple of 4");
            need = (size_t)bh * (bw >> 2) * 3; break;
    case 6: need = (size_t)bw * bh; break;
    case 2: case 3: if (!mask || !maskBBox || maskBBox[2] <= 0) return yk_fail(c, YK_ERR_BAD_ARG, "mask mode needs the decoded mipmap mask"); break;
    default: return yk_fail(c, YK_ERR_BAD_ARG, "alpha mode not decodable");        // 0 (1 bit + mask) and 7
    }
    if (n < need) return yk_fail(c, YK_ERR_RANGE, "alpha payload shorter than its box");
    YK_HIP(c, hipSetDevice(c->device));
    const size_t plane = (size_t)W * H;
    YK_HIP(c, c->dAlpha.reserve(c->stream, plane));
    c->dAlphaValid = false; c->dAlphaBatch = false;
    const size_t oPay = 0, oMask = (n + 255) & ~(size_t)255, oRows = oMask + ((maskBytes + 255) & ~(size_t)255);
    const size_t scratch = oRows + ((size_t)bh * 2 + 2) * sizeof(uint32_t) + 64;
    YK_HIP(c, c->dAvScratch.reserve(c->stream, scratch));
    uint8_t* S = c->dAvScratch;
    if (n) YK_HIP(c, hipMemcpyAsync(S + oPay, payload, n, hipMemcpyHostToDevice, c->stream));
    if (mode == 2 || mode == 3) {
        if (maskBytes) YK_HIP(c, hipMemcpyAsync(S + oMask, mask, maskBytes, hipMemcpyHostToDevice, c->stream));
        uint32_t* rowCnt = reinterpret_cast<uint32_t*>(S + oRows);
        uint32_t* rowStart = rowCnt + bh;
        const uint32_t stride = (uint32_t)maskBBox[2];
        const uint32_t base = (uint32_t)(bx - maskBBox[0]) + stride * (uint32_t)(by - maskBBox[1]);
        YK_HIP(c, hipMemsetAsync(c->dAlpha, 0, plane, c->stream));
        hipLaunchKernelGGL(yk_av_rowcount_kernel, dim3(bh), dim3(64), 0, c->stream, S + oMask, maskBytes, base, stride, bw, rowCnt);
        hipLaunchKernelGGL(yk_av_rowscan_kernel, dim3(1), dim3(1024), 0, c->stream, rowCnt, bh, rowStart);
        YK_HIP(c, hipGetLastError());
        uint32_t total = 0;
        YK_HIP(c, hipMemcpyAsync(&total, rowStart + bh, sizeof total, hipMemcpyDeviceToHost, c->stream));
        YK_HIP(c, hipStreamSynchronize(c->stream));
        const size_t needM = ((size_t)total * 6 + 7) / 8;
        if (n < needM) return yk_fail(c, YK_ERR_RANGE, "alpha payload shorter than the mask selects");
        hipLaunchKernelGGL(yk_av_maskdecode_kernel, dim3(bh), dim3(64), 0, c->stream, S + oPay, n, S + oMask, maskBytes, base, stride, bx, by, bw,
                           mode == 3 ? 1 : 0, rowStart, W, c->dAlpha);
    } else {
        hipLaunchKernelGGL((W & 15) ? yk_av_decode_kernel<true> : yk_av_decode_kernel<false>, dim3((unsigned)((plane / 16 + 255) / 256)), dim3(256), 0,
                           c->stream, S + oPay, n, mode, refQuirk ? 1 : 0, bx, by, bw, bh, W, H, c->dAlpha);
    }
    YK_HIP(c, hipGetLastError());
    c->dAlphaValid = true;
    return YK_OK;
}

int yk_decode_alpha_plane(yk_ctx* c, uint8_t* hostOut, size_t cap) {
    if (!c || !hostOut) return YK_ERR_BAD_ARG;
    if (!c->dAlphaValid) return yk_fail(c, YK_ERR_STATE, "yk_decode_alpha first");
    const size_t plane = (size_t)c->dw * c->dh;
    if (cap < plane) return yk_fail(c, YK_ERR_RANGE, "alpha buffer too small");
    YK_HIP(c, hipSetDevice(c->device));
    YK_HIP(c, hipMemcpyAsync(hostOut, yk_dec_alpha_cur(c), plane, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

}  // extern "C"

// ---- encode, host side: yk_alpha_values is yk_alpha_values_batch's path with one frame ---------------------------------------------------------
static unsigned long long yk_ave_frame_elems(const yk_ctx* c) { return c->nFrames > 1 ? c->fs.plane : 0; }
// 16-byte loads: the base aligned to 16, the row and the frame pitch multiples of 4 samples
static bool yk_ave_vec(const yk_ctx* c) {
    return ((reinterpret_cast<uintptr_t>(c->B.plane[3]) & 15) == 0) && ((c->strideElems & 3) == 0) && ((yk_ave_frame_elems(c) & 3) == 0);
}
// Box and class of every frame of the handle: st = the 8 state words per frame after the class kernel, tab = one record per frame that has a
// box, also in avTab; the frames' 8-bit payloads are in their slots of avPay.  Two launches, two blocking read-backs and one table upload
// whatever nFrames is.  The entry points have checked the handle; the only failure of its own is "alpha box beyond the image"
static int yk_ave_classify(yk_ctx* c, std::vector<int32_t>& st, std::vector<YkAvFrame>& tab) {
    const int N = c->nFrames, W = c->fullW, H = c->fullH;
    YK_HIP(c, c->avState.reserve(c->stream, (size_t)N * 8));
    st.resize((size_t)N * 8);
    for (int f = 0; f < N; f++) { int32_t* s = &st[(size_t)f * 8]; s[0] = s[1] = INT_MAX; s[2] = s[3] = -1; s[4] = s[5] = s[6] = s[7] = 0; }
    YK_HIP(c, hipMemcpyAsync(c->avState, st.data(), st.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const int32_t* alpha = c->B.plane[3];
    const unsigned long long fe = yk_ave_frame_elems(c);
    const bool vec = yk_ave_vec(c);
    // the search region is at most the image; the kernel clamps it to the bounds the alpha stage left on the device
    hipLaunchKernelGGL(vec ? yk_ave_box_batch_kernel<true> : yk_ave_box_batch_kernel<false>,
                       dim3((unsigned)((W / 4 + 255) / 256), (unsigned)((H + YK_AV_ROWS - 1) / YK_AV_ROWS), (unsigned)N), dim3(256), 0, c->stream, alpha, fe,
                       c->strideElems, c->B.bounds + c->boundsOff, W, H, c->avState);
    YK_HIP(c, hipGetLastError());
    YK_HIP(c, hipMemcpyAsync(st.data(), c->avState, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));                                           // readback 1: every frame's box sizes every later launch
    // the payload slots back to back, each on a multiple of 16: bw * bh bytes of the box rounded to 4 (the 1-bit payload of the box re-aligned
    // to 8 is never longer)
    tab.clear();
    size_t total = 0;
    int maxW = 0, maxH = 0;
    for (int f = 0; f < N; f++) {
        const int32_t* s = &st[(size_t)f * 8];
        if (s[2] < 0) continue;                                                           // empty box: isAll0 and isAll1 stay true, no chunk
        const int bL = (s[0] >> 2) << 2, bR = ((s[2] + 1 + 3) >> 2) << 2, bT = s[1], bB = s[3] + 1;   // :1465-1466
        // the one bounds check, for the box re-aligned to 8 too (yk_ave_chunk): W is a multiple of 8 (yk_set_image), so ((bR + 7) & ~7) > W is bR > W
        if (bL < 0 || bT < 0 || bR > W || bB > H || ((bR + 7) & ~7) > W) return yk_fail(c, YK_ERR_STATE, "alpha box beyond the image");
        YkAvFrame r;
        r.bL = bL; r.bT = bT; r.bw = bR - bL; r.bh = bB - bT; r.off = total; r.frame = f; r.pad = 0;
        tab.push_back(r);
        total = (total + (size_t)r.bw * r.bh + 15) & ~(size_t)15;
        maxW = max(maxW, r.bw); maxH = max(maxH, r.bh);
    }
    if (tab.empty()) return YK_OK;
    YK_HIP(c, c->avPay.reserve(c->stream, total));
    const size_t tabBytes = tab.size() * sizeof(YkAvFrame);
    if (c->avTab.cap < tabBytes) YK_HIP(c, c->avTab.reserve(c->stream, (size_t)N * sizeof(YkAvFrame)));      // grown when the records do not fit, then for every frame
    YK_HIP(c, hipMemcpyAsync(c->avTab, tab.data(), tabBytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(vec ? yk_ave_class_batch_kernel<true> : yk_ave_class_batch_kernel<false>,
                       dim3((unsigned)((maxW / 4 + 255) / 256), (unsigned)maxH, (unsigned)tab.size()), dim3(256), 0, c->stream, alpha, fe, c->strideElems,
                       reinterpret_cast<const YkAvFrame*>(c->avTab.p), c->avPay, c->avState);
    YK_HIP(c, hipGetLastError());
    YK_HIP(c, hipMemcpyAsync(st.data(), c->avState, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));                                           // readback 2: every frame's class decides its payload
    return YK_OK;
}
// The class decision of ProcessAlpha(true), the only copy: a record and its frame's two flags -> the chunk's mode and box in `o`, its payload
// length returned.  Analog: IS_8_BIT_FULL, the slot as the class kernel wrote it.  All 255: no chunk, o.mode stays -1.  Binary: IS_1_BIT_FULL
// on the box re-aligned to 8, which yk_ave_pack1_batch_kernel writes into the slot
static size_t yk_ave_chunk(const YkAvFrame& r, const int32_t* s, yk_alpha_info& o) {
    const bool analog = s[4] != 0, all1 = s[5] == 0;
    int bL = r.bL, bw = r.bw;
    size_t bytes;
    if (analog) { o.mode = 6; bytes = (size_t)bw * r.bh; }
    else if (all1) return 0;
    else {
        const int bR = ((bL + bw + 7) >> 3) << 3;
        bL = (bL >> 3) << 3; bw = bR - bL;
        o.mode = 1; bytes = (size_t)(bw >> 3) * r.bh;
    }
    o.bbox[0] = bL; o.bbox[1] = r.bT; o.bbox[2] = bw; o.bbox[3] = r.bh; o.rawSize = (uint32_t)bytes;
    return bytes;
}
// maxBytes1 = the longest 1-bit payload among the nBox records in avTab (sizes the grid)
static int yk_ave_pack1(yk_ctx* c, size_t nBox, size_t maxBytes1) {
    hipLaunchKernelGGL(yk_ave_pack1_batch_kernel, dim3((unsigned)((maxBytes1 + 255) / 256), 1, (unsigned)nBox), dim3(256), 0, c->stream, c->B.plane[3],
                       yk_ave_frame_elems(c), c->strideElems, reinterpret_cast<const YkAvFrame*>(c->avTab.p), c->avPay, c->avState);
    YK_HIP(c, hipGetLastError());
    return YK_OK;
}

extern "C" {

int yk_alpha_values(yk_ctx* c, int force8Bit, yk_alpha_info* out, uint8_t* hostPayload, size_t cap, size_t* n) {
    if (!c || !out) return YK_ERR_BAD_ARG;
    out->mode = -1; out->bbox[0] = out->bbox[1] = out->bbox[2] = out->bbox[3] = 0; out->rawSize = 0;
    if (n) *n = 0;
    if (c->nPlanes != 4) return YK_OK;                                                    // no alpha: no chunk (:1674-1680)
    if (!c->alphaFinished) return yk_fail(c, YK_ERR_STATE, "yk_alpha_reject + yk_alpha_finish first");
    if (c->nFrames != 1 || c->y0 != 0 || c->h != c->fullH) return yk_fail(c, YK_ERR_STATE, "yk_alpha_values works on a whole single image");
    const int W = c->fullW, H = c->fullH;
    YK_HIP(c, hipSetDevice(c->device));
    c->avBatchValid = false;                                                              // the batch payloads share avState / avPay / avTab: no slot is published here
    std::vector<int32_t> st;
    std::vector<YkAvFrame> tab;
    { const int rc = yk_ave_classify(c, st, tab); if (rc) return rc; }
    if (tab.empty()) return YK_OK;                                                        // empty box: no chunk
    const YkAvFrame& r = tab[0];                                                          // its slot is at avPay + 0
    yk_alpha_info o = *out;
    size_t bytes = yk_ave_chunk(r, &st[0], o);
    if (o.mode < 0) return YK_OK;                                                         // all 255: no chunk
    const uint8_t* src = c->avPay;
    if (o.mode == 1) {
        const int rc = yk_ave_pack1(c, 1, bytes); if (rc) return rc;
    } else if (!force8Bit) {                                                              // analog: IS_6_BIT_USEMIPMAPMASK_INVERSE from the u8 box in the slot
        const YkFrameView V = yk_frame(c);
        const int bL = r.bL, bT = r.bT, bw = r.bw, bh = r.bh, bR = bL + bw, bB = bT + bh;
        if (!V.keep || (bL & 3) || (bw & 3)) return yk_fail(c, YK_ERR_STATE, "6-bit alpha: no keep flags or a box not aligned to 4");
        const int nb = ((bB - 1) >> 4) - (bT >> 4) + 1, ncol = ((bR - 1) >> 4) - (bL >> 4) + 1;
        const size_t nU32 = (size_t)nb * ncol + 3 * (size_t)nb + 1;
        const size_t oPay = (nU32 * sizeof(uint32_t) + 255) & ~(size_t)255, payCap = (size_t)(bw >> 2) * 3 * bh;
        YK_HIP(c, c->av6.reserve(c->stream, oPay + payCap));
        uint32_t* colPre = reinterpret_cast<uint32_t*>(c->av6.p);
        uint32_t* bandS = colPre + (size_t)nb * ncol;
        uint32_t* bandCnt = bandS + nb;
        uint32_t* bandStart = bandCnt + nb;
        uint8_t* pay6 = c->av6 + oPay;
        const int32_t* bounds = V.bounds + c->boundsOff;
        hipLaunchKernelGGL(yk_ave_band_kernel, dim3((unsigned)nb), dim3(64), 0, c->stream, V.keep, c->mtW, c->mtH, bounds, W, H, bL, bT, bR, bB, ncol, colPre,
                           bandS, bandCnt);
        hipLaunchKernelGGL(yk_av_rowscan_kernel, dim3(1), dim3(1024), 0, c->stream, bandCnt, nb, bandStart);
        hipLaunchKernelGGL(yk_ave_pack6_kernel, dim3((unsigned)((bw / 4 + 255) / 256), (unsigned)bh), dim3(256), 0, c->stream, c->avPay, bL, bT, bw, bh, V.keep,
                           c->mtW, c->mtH, bounds, W, H, ncol, nb, colPre, bandS, bandStart, pay6, payCap);
        YK_HIP(c, hipGetLastError());
        uint32_t total = 0;
        YK_HIP(c, hipMemcpyAsync(&total, bandStart + nb, sizeof total, hipMemcpyDeviceToHost, c->stream));
        YK_HIP(c, hipStreamSynchronize(c->stream));                                       // readback 3: the selected count sizes the payload
        static const size_t tail[4] = { 0, 1, 2, 3 };
        bytes = (size_t)(total >> 2) * 3 + tail[total & 3];                                // :1549-1551 (total is a multiple of 4 here)
        if (bytes > payCap) return yk_fail(c, YK_ERR_STATE, "6-bit alpha: selected count beyond the box");
        o.mode = 3; o.rawSize = (uint32_t)bytes; src = pay6;
    }
    *out = o;
    if (n) *n = bytes;
    if (hostPayload) {
        if (cap < bytes) return yk_fail(c, YK_ERR_RANGE, "alpha payload buffer too small");
        YK_HIP(c, hipMemcpyAsync(hostPayload, src, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

// ProcessAlpha(true) for every frame of the handle: at most three launches, two read-backs and one record table per batch
int yk_alpha_values_batch(yk_ctx* c, int force8Bit, yk_alpha_info* infos) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!infos) return yk_refuse(c, YK_ERR_BAD_ARG, "infos is NULL");
    if (!force8Bit) return yk_refuse(c, YK_ERR_BAD_ARG, "the 6-bit mask mode (force8Bit = 0) is not batched: it needs every frame's mask selection");
    const int N = c->nFrames;
    if (c->nPlanes == 4) {
        if (!c->alphaFinished) return yk_refuse(c, YK_ERR_STATE, "the alpha stage first: yk_encode_batch, or yk_alpha_reject + yk_alpha_finish");
        if (c->y0 != 0 || c->h != c->fullH) return yk_refuse(c, YK_ERR_STATE, "yk_alpha_values_batch works on whole images, not on a stripe");
        if (!c->B.plane[3] || (N > 1 && c->fs.plane == 0)) return yk_refuse(c, YK_ERR_STATE, "bind planes first");
    }
    for (int f = 0; f < N; f++) { infos[f].mode = -1; infos[f].bbox[0] = infos[f].bbox[1] = infos[f].bbox[2] = infos[f].bbox[3] = 0; infos[f].rawSize = 0; }
    c->avBatchValid = false;
    c->avBatch.assign((size_t)N, yk_ctx::AvSlot{ -1, 0, 0 });
    if (c->nPlanes != 4) { c->avBatchValid = true; return YK_OK; }                        // no alpha: no chunk in any frame (:1674-1680)
    YK_HIP(c, hipSetDevice(c->device));
    std::vector<int32_t> st;
    std::vector<YkAvFrame> tab;
    { const int rc = yk_ave_classify(c, st, tab); if (rc) return rc; }
    size_t maxBytes1 = 0;
    for (const YkAvFrame& r : tab) {
        yk_alpha_info& o = infos[r.frame];
        const size_t bytes = yk_ave_chunk(r, &st[(size_t)r.frame * 8], o);
        if (o.mode < 0) continue;                                                         // all 255: no chunk
        if (o.mode == 1) maxBytes1 = bytes > maxBytes1 ? bytes : maxBytes1;
        c->avBatch[(size_t)r.frame] = yk_ctx::AvSlot{ o.mode, (size_t)r.off, bytes };
    }
    if (maxBytes1) { const int rc = yk_ave_pack1(c, tab.size(), maxBytes1); if (rc) return rc; }
    c->avBatchValid = true;
    return YK_OK;
}

// ProcessAlpha(force8Bit[f] != 0) for every frame of the handle: yk_alpha_values_batch's path, and for the frames classed analog whose force8Bit is 0
// the three 6-bit launches over all of them, one more record table and the read-back of their selected counts
int yk_alpha_values_mask_batch(yk_ctx* c, const uint8_t* force8Bit, yk_alpha_info* infos) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!infos) return yk_refuse(c, YK_ERR_BAD_ARG, "infos is NULL");
    const int N = c->nFrames, W = c->fullW, H = c->fullH;
    if (c->nPlanes == 4) {
        if (!c->alphaFinished) return yk_refuse(c, YK_ERR_STATE, "the alpha stage first: yk_encode_batch, or yk_alpha_reject + yk_alpha_finish");
        if (c->y0 != 0 || c->h != c->fullH) return yk_refuse(c, YK_ERR_STATE, "yk_alpha_values_mask_batch works on whole images, not on a stripe");
        if (!c->B.plane[3] || (N > 1 && c->fs.plane == 0)) return yk_refuse(c, YK_ERR_STATE, "bind planes first");
        if (!c->B.keep || !c->B.bounds) return yk_refuse(c, YK_ERR_STATE, "6-bit alpha: the handle has no keep flags");
    }
    for (int f = 0; f < N; f++) { infos[f].mode = -1; infos[f].bbox[0] = infos[f].bbox[1] = infos[f].bbox[2] = infos[f].bbox[3] = 0; infos[f].rawSize = 0; }
    c->avBatchValid = false;
    c->avBatch.assign((size_t)N, yk_ctx::AvSlot{ -1, 0, 0 });
    if (c->nPlanes != 4) { c->avBatchValid = true; return YK_OK; }                        // no alpha: no chunk in any frame (:1674-1680)
    YK_HIP(c, hipSetDevice(c->device));
    std::vector<int32_t> st;
    std::vector<YkAvFrame> tab;
    { const int rc = yk_ave_classify(c, st, tab); if (rc) return rc; }
    // the class decision of every frame; an analog frame with force8Bit = 0 gets a record: its 6-bit slot ((bw / 4) * 3 * bh bytes, on a multiple of
    // 16) and its region of the u32 arena
    std::vector<YkAv6Rec> recs;
    std::vector<int> frameOf;                                                             // record -> frame
    size_t maxBytes1 = 0, paySize = 0, arena = 0;
    int maxNb = 0, maxBw = 0, maxBh = 0;
    for (const YkAvFrame& r : tab) {
        yk_alpha_info& o = infos[r.frame];
        const size_t bytes = yk_ave_chunk(r, &st[(size_t)r.frame * 8], o);
        if (o.mode < 0) continue;                                                         // all 255: no chunk
        if (o.mode == 1) maxBytes1 = bytes > maxBytes1 ? bytes : maxBytes1;
        c->avBatch[(size_t)r.frame] = yk_ctx::AvSlot{ o.mode, (size_t)r.off, bytes };
        if (o.mode != 6 || (force8Bit && force8Bit[r.frame])) continue;
        const YkFrameView V = yk_frame(c, r.frame);
        YkAv6Rec q;
        q.keep = V.keep; q.bounds = V.bounds + c->boundsOff; q.box = c->avPay + r.off; q.out = nullptr;
        q.bL = r.bL; q.bT = r.bT; q.bR = r.bL + r.bw; q.bB = r.bT + r.bh;
        q.nb = ((q.bB - 1) >> 4) - (q.bT >> 4) + 1; q.ncol = ((q.bR - 1) >> 4) - (q.bL >> 4) + 1;
        q.cap = (unsigned long long)(r.bw >> 2) * 3 * r.bh; q.arena = arena;
        arena += (size_t)q.nb * q.ncol + 3 * (size_t)q.nb + 1;
        c->avBatch[(size_t)r.frame] = yk_ctx::AvSlot{ 3, paySize, 0 };                    // the slot's offset behind the tables: added below
        paySize = (paySize + (size_t)q.cap + 15) & ~(size_t)15;
        maxNb = max(maxNb, q.nb); maxBw = max(maxBw, r.bw); maxBh = max(maxBh, r.bh);
        recs.push_back(q); frameOf.push_back(r.frame);
    }
    if (maxBytes1) { const int rc = yk_ave_pack1(c, tab.size(), maxBytes1); if (rc) return rc; }
    const size_t n6 = recs.size();
    if (n6) {
        // av6: the record table, the n6 totals, the u32 arena, the 6-bit slots
        const size_t oTot = (n6 * sizeof(YkAv6Rec) + 15) & ~(size_t)15, oArena = (oTot + n6 * sizeof(uint32_t) + 15) & ~(size_t)15;
        const size_t oPay = (oArena + arena * sizeof(uint32_t) + 255) & ~(size_t)255;
        YK_HIP(c, c->av6.reserve(c->stream, oPay + paySize));
        for (size_t k = 0; k < n6; k++) {
            yk_ctx::AvSlot& s = c->avBatch[(size_t)frameOf[k]];
            s.off += oPay; recs[k].out = c->av6 + s.off;
        }
        YK_HIP(c, hipMemcpyAsync(c->av6, recs.data(), n6 * sizeof(YkAv6Rec), hipMemcpyHostToDevice, c->stream));
        const YkAv6Rec* dTab = reinterpret_cast<const YkAv6Rec*>(c->av6.p);
        uint32_t* dTot = reinterpret_cast<uint32_t*>(c->av6 + oTot);
        uint32_t* u32s = reinterpret_cast<uint32_t*>(c->av6 + oArena);
        hipLaunchKernelGGL(yk_ave_band_batch_kernel, dim3((unsigned)maxNb, 1, (unsigned)n6), dim3(64), 0, c->stream, dTab, c->mtW, c->mtH, W, H, u32s);
        hipLaunchKernelGGL(yk_ave_bandscan_batch_kernel, dim3(1, 1, (unsigned)n6), dim3(64), 0, c->stream, dTab, u32s, dTot);
        hipLaunchKernelGGL(yk_ave_pack6_batch_kernel, dim3((unsigned)((maxBw / 4 + 255) / 256), (unsigned)maxBh, (unsigned)n6), dim3(256), 0, c->stream, dTab,
                           c->mtW, c->mtH, W, H, u32s);
        YK_HIP(c, hipGetLastError());
        std::vector<uint32_t> totals(n6);
        YK_HIP(c, hipMemcpyAsync(totals.data(), dTot, n6 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        YK_HIP(c, hipStreamSynchronize(c->stream));                                       // readback 3: the selected counts size the payloads
        for (size_t k = 0; k < n6; k++) {
            const uint32_t total = totals[k];
            static const size_t tail[4] = { 0, 1, 2, 3 };
            const size_t bytes = (size_t)(total >> 2) * 3 + tail[total & 3];               // :1549-1551 (total is a multiple of 4 here)
            if (bytes > (size_t)recs[k].cap) return yk_fail(c, YK_ERR_STATE, "6-bit alpha: selected count beyond the box");
            c->avBatch[(size_t)frameOf[k]].bytes = bytes;
            infos[frameOf[k]].mode = 3; infos[frameOf[k]].rawSize = (uint32_t)bytes;
        }
    }
    c->avBatchValid = true;
    return YK_OK;
}

int yk_alpha_payload_device(yk_ctx* c, int frame, const uint8_t** dev, size_t* nBytes) {
    if (!c) return YK_ERR_BAD_ARG;
    if (dev) *dev = nullptr;
    if (nBytes) *nBytes = 0;
    if (!dev || !nBytes) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL result pointer");
    if (!c->avBatchValid) return yk_refuse(c, YK_ERR_STATE, "yk_alpha_values_batch first");
    if (frame < 0 || frame >= (int)c->avBatch.size()) return yk_refuse(c, YK_ERR_BAD_ARG, "frame out of range");
    const yk_ctx::AvSlot& s = c->avBatch[(size_t)frame];
    if (s.mode < 0) return YK_OK;
    *dev = (s.mode == 3 ? c->av6.p : c->avPay.p) + s.off; *nBytes = s.bytes;   // mode 3: the 6-bit slot of yk_alpha_values_mask_batch
    return YK_OK;
}

int yk_alpha_payload(yk_ctx* c, int frame, uint8_t* hostOut, size_t cap, size_t* nBytes) {
    if (!c) return YK_ERR_BAD_ARG;
    const uint8_t* dev = nullptr; size_t n = 0;
    if (nBytes) *nBytes = 0;
    { const int rc = yk_alpha_payload_device(c, frame, &dev, &n); if (rc) return rc; }
    if (nBytes) *nBytes = n;
    if (!n) return YK_OK;
    if (!hostOut || cap < n) return yk_refuse(c, YK_ERR_RANGE, "alpha payload buffer too small");
    YK_HIP(c, hipSetDevice(c->device));
    YK_HIP(c, hipMemcpyAsync(hostOut, dev, n, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    return YK_OK;
}

// The 'ALPM' plane of every frame of a decode batch; records through the pinned ring + an HBM table, no host synchronisation.  mip* == nullptr:
// yk_decode_alpha_batch_device (one launch, the mask modes are refused).  Otherwise the frames of modes 2 / 3 get a zero plane from that launch
// (a record with an empty box) and their values from three more launches over all of them: row count, per-frame scan, decode
static int yk_av_decode_batch(yk_ctx* c, const int32_t* modes, const int32_t* bboxes, const uint8_t* const* devPayload, const size_t* payBytes,
                              const uint8_t* const* devMipBits, const size_t* mipBytes, const int32_t* mipBoxes, bool masks, int noChunkAlpha) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!modes || !bboxes || !devPayload || !payBytes || (masks && (!devMipBits || !mipBytes || !mipBoxes))) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL table");
    if (noChunkAlpha < 0 || noChunkAlpha > 255) return yk_refuse(c, YK_ERR_BAD_ARG, "noChunkAlpha must be 0..255");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_begin_batch first");
    const int N = c->dFrames, W = c->dw, H = c->dh;
    const long long tileGrid = (long long)((W + 15) >> 4) * ((H + 15) >> 4);
    int nMask = 0, maxBh = 0;
    size_t rowWords = 0;
    for (int f = 0; f < N; f++) {
        const int mode = modes[f];
        if (mode == -1) continue;
        const int bx = bboxes[4 * f], by = bboxes[4 * f + 1], bw = bboxes[4 * f + 2], bh = bboxes[4 * f + 3];
        if (bx < 0 || by < 0 || bw <= 0 || bh <= 0 || bx >= W || by >= H || bx + bw > W || by + bh > H) return yk_refuse(c, YK_ERR_BAD_ARG, "alpha box outside the image");
        if (masks) {
            const long long tw = mipBoxes[4 * f + 2], th = mipBoxes[4 * f + 3];
            if (tw < 0 || th < 0 || tw * th > tileGrid) return yk_refuse(c, YK_ERR_BAD_ARG, "'MIPM' tile box negative or larger than the image's tile grid");
        }
        size_t need = 0;
        switch (mode) {
        case 1: if (bw & 7) return yk_refuse(c, YK_ERR_BAD_ARG, "1-bit alpha box width not a multiple of 8");
                need = (size_t)bh * (bw >> 3); break;
        case 4: case 5: if (bw & 3) return yk_refuse(c, YK_ERR_BAD_ARG, "6-bit alpha box width not a multiple of 4");
                need = (size_t)bh * (bw >> 2) * 3; break;
        case 6: need = (size_t)bw * bh; break;
        case 2: case 3: {
            if (!masks) return yk_refuse(c, YK_ERR_BAD_ARG, "the mask modes 2 and 3 are not batched: they need every frame's decoded mipmap mask");
            if (mipBoxes[4 * f + 2] == 0 || !devMipBits[f]) return yk_refuse(c, YK_ERR_BAD_ARG, "mask mode on a frame without a 'MIPM' bitmap");
            if (bw & 3) return yk_refuse(c, YK_ERR_BAD_ARG, "6-bit alpha box width not a multiple of 4");
            const size_t tiles = (size_t)mipBoxes[4 * f + 2] * (size_t)mipBoxes[4 * f + 3];
            if (mipBytes[f] < (tiles + 7) / 8) return yk_refuse(c, YK_ERR_RANGE, "'MIPM' bitmap shorter than its tile box");
            nMask++; maxBh = max(maxBh, bh); rowWords += 2 * (size_t)bh + 1;
            break; }
        default: return yk_refuse(c, YK_ERR_BAD_ARG, "alpha mode not decodable");          // 0 (1 bit + mask), 7, anything else
        }
        if (!devPayload[f] && payBytes[f]) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL alpha payload with a length");
        if (payBytes[f] < need) return yk_refuse(c, YK_ERR_RANGE, "alpha payload shorter than its box");
    }
    YK_HIP(c, hipSetDevice(c->device));
    const size_t plane = (size_t)W * H, stride = (plane + 15) & ~(size_t)15;
    if (c->dAlpha.cap < stride * N) c->dAlphaValid = false;
    YK_HIP(c, c->dAlpha.reserve(c->stream, stride * N));
    const size_t oMask = (size_t)N * sizeof(YkAvDecFrame), tabBytes = oMask + (size_t)nMask * sizeof(YkAvMaskFrame);
    const size_t oRows = (tabBytes + 255) & ~(size_t)255;
    YK_HIP(c, c->dAvScratch.reserve(c->stream, oRows + rowWords * sizeof(uint32_t)));
    if (nMask) YK_HIP(c, c->dAvStatus.reserve(c->stream, 1024));                           // the most frames a batch can have: never re-made
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, tabBytes, &slot, &host); if (rc) return rc; }
    YkAvDecFrame* tab = static_cast<YkAvDecFrame*>(host);
    YkAvMaskFrame* mtab = reinterpret_cast<YkAvMaskFrame*>(static_cast<uint8_t*>(host) + oMask);
    c->dAvMaskFrames.clear();
    size_t rowsAt = 0;
    for (int f = 0; f < N; f++) {
        YkAvDecFrame& r = tab[f];
        const bool masked = modes[f] == 2 || modes[f] == 3;
        r.mode = masked ? 6 : modes[f]; r.pay = (r.mode < 0 || masked) ? nullptr : devPayload[f]; r.n = (r.mode < 0 || masked) ? 0 : payBytes[f];
        const bool has = r.mode >= 0 && !masked;                                            // a masked frame: an empty box, every pixel 0
        r.bx = has ? bboxes[4 * f] : 0; r.by = has ? bboxes[4 * f + 1] : 0; r.bw = has ? bboxes[4 * f + 2] : 0; r.bh = has ? bboxes[4 * f + 3] : 0;
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        if (!masked) continue;
        YkAvMaskFrame& m = mtab[c->dAvMaskFrames.size()];
        m.pay = devPayload[f]; m.n = payBytes[f]; m.bits = devMipBits[f];
        m.tbw = (uint32_t)mipBoxes[4 * f + 2]; m.nq = 4u * m.tbw * (uint32_t)mipBoxes[4 * f + 3];
        m.stride = m.tbw << 4;                                                              // maskBBox = the tile box << 4, u32 arithmetic as the reference's mipmapPos
        m.base = ((uint32_t)bboxes[4 * f] - (uint32_t)mipBoxes[4 * f] * 16u) + m.stride * ((uint32_t)bboxes[4 * f + 1] - (uint32_t)mipBoxes[4 * f + 1] * 16u);
        m.bx = bboxes[4 * f]; m.by = bboxes[4 * f + 1]; m.bw = bboxes[4 * f + 2]; m.bh = bboxes[4 * f + 3];
        m.inv = modes[f] == 3 ? 1 : 0; m.frame = f; m.oRows = (uint32_t)rowsAt; m.pad = 0;
        rowsAt += 2 * (size_t)m.bh + 1;
        c->dAvMaskFrames.push_back(f);
    }
    c->dAlphaValid = false;
    { const int rc = yk_dec_table_upload(c, slot, c->dAvScratch, tabBytes); if (rc) return rc; }
    hipLaunchKernelGGL((W & 15) ? yk_av_decode_batch_kernel<true> : yk_av_decode_batch_kernel<false>, dim3((unsigned)((plane / 16 + 255) / 256), (unsigned)N),
                       dim3(256), 0, c->stream, reinterpret_cast<const YkAvDecFrame*>(c->dAvScratch.p), W, H, c->dAlpha, stride,
                       (uint32_t)noChunkAlpha * 0x01010101u);
    if (nMask) {
        const YkAvMaskFrame* dTab = reinterpret_cast<const YkAvMaskFrame*>(c->dAvScratch + oMask);
        uint32_t* rows = reinterpret_cast<uint32_t*>(c->dAvScratch + oRows);
        const dim3 perRow((unsigned)maxBh, (unsigned)nMask);
        hipLaunchKernelGGL(yk_av_rowcount_batch_kernel, perRow, dim3(64), 0, c->stream, dTab, rows);
        hipLaunchKernelGGL(yk_av_rowscan_batch_kernel, dim3((unsigned)nMask), dim3(1024), 0, c->stream, dTab, rows, c->dAvStatus.p);
        hipLaunchKernelGGL(yk_av_maskdecode_batch_kernel, perRow, dim3(64), 0, c->stream, dTab, rows, W, c->dAlpha.p, stride);
    }
    YK_HIP(c, hipGetLastError());
    c->dAlphaValid = true; c->dAlphaBatch = true; c->dAlphaStride = stride;
    return YK_OK;
}

int yk_decode_alpha_batch_device(yk_ctx* c, const int32_t* modes, const int32_t* bboxes, const uint8_t* const* devPayload, const size_t* payBytes,
                                 int noChunkAlpha) {
    return yk_av_decode_batch(c, modes, bboxes, devPayload, payBytes, nullptr, nullptr, nullptr, false, noChunkAlpha);
}

int yk_decode_alpha_mask_batch_device(yk_ctx* c, const int32_t* modes, const int32_t* bboxes, const uint8_t* const* devPayload, const size_t* payBytes,
                                      const uint8_t* const* devMipBits, const size_t* mipBytes, const int32_t* mipBoxes, int noChunkAlpha) {
    return yk_av_decode_batch(c, modes, bboxes, devPayload, payBytes, devMipBits, mipBytes, mipBoxes, true, noChunkAlpha);
}

// the counterpart of yk_palette_decode_status: what the mask call could not know without a read-back
int yk_decode_alpha_batch_status(yk_ctx* c, int32_t* out) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!out) return yk_refuse(c, YK_ERR_BAD_ARG, "out is NULL");
    if (!c->dAlphaValid || !c->dAlphaBatch) return yk_refuse(c, YK_ERR_STATE, "yk_decode_alpha_mask_batch_device first: the batch has no decoded alpha planes");
    YK_HIP(c, hipSetDevice(c->device));
    for (int f = 0; f < c->dFrames; f++) out[f] = 0;
    const size_t nMask = c->dAvMaskFrames.size();
    std::vector<int32_t> st(nMask);
    if (nMask) YK_HIP(c, hipMemcpyAsync(st.data(), c->dAvStatus, nMask * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < nMask; i++) out[c->dAvMaskFrames[i]] = st[i];
    return YK_OK;
}

}  // extern "C"

// ---- 'MIPM' bitmaps of every frame (yk_alpha_bitmaps_batch) -------------------------------------------------------------------------------------
// The rule is yk_alpha_bitmap's (EncoderContext.cpp:1317-1327): inside the box of kept tiles, in 16-pixel tiles {bx0, by0, tw, th}, bit y * tw + x,
// LSB first, is the keep flag of tile (bx0 + x, by0 + y); no bits when the box is the whole image or no tile is kept.  blockIdx.y = frame; a thread
// produces one byte of its frame's slot, i.e. the flags of 8 consecutive bit positions, which cross tile rows wherever tw is no multiple of 8; it
// divides once and then steps.  The box and the frame's flags are read through uniform loads.  Every byte of the slot is written, zeros behind the bits.
namespace {
#define YK_MIP_THREADS 256
__global__ __launch_bounds__(YK_MIP_THREADS) void yk_mip_bits_batch_kernel(const uint8_t* __restrict__ keep, unsigned long long keepStride, const int32_t* __restrict__ bounds,
                                                                           int W, int H, int mtW, int mtH, uint32_t slot, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * YK_MIP_THREADS + threadIdx.x;
    if (i >= slot) return;
    const uint32_t f = blockIdx.y;
    const int32_t* b = bounds + (size_t)f * 16;
    const int b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    const int bx0 = b0 >> 4, by0 = b1 >> 4, tw = (b2 >> 4) - bx0, th = (b3 >> 4) - by0;
    const bool none = (b0 == 0 && b1 == 0 && b2 == W && b3 == H) || b2 < b0 || tw <= 0 || th <= 0 || bx0 < 0 || by0 < 0;
    const uint32_t nBits = none ? 0u : (uint32_t)tw * (uint32_t)th;
    const uint8_t* __restrict__ k = keep + (size_t)f * keepStride;
    uint32_t v = 0, bp = i * 8u;
    if (bp < nBits) {
        uint32_t y = bp / (uint32_t)tw, x = bp - y * (uint32_t)tw;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t mx = (uint32_t)bx0 + x, my = (uint32_t)by0 + y;
            if (bp + j < nBits && mx < (uint32_t)mtW && my < (uint32_t)mtH && k[(size_t)my * mtW + mx]) v |= 1u << j;
            if (++x == (uint32_t)tw) { x = 0; y++; }
        }
    }
    out[(size_t)f * slot + i] = (uint8_t)v;
}
}  // namespace

extern "C" {

int yk_alpha_bitmaps_batch(yk_ctx* c, yk_mip_info* infos) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!infos) return yk_refuse(c, YK_ERR_BAD_ARG, "infos is NULL");
    if (c->fullW <= 0 || c->fullH <= 0) return yk_refuse(c, YK_ERR_STATE, "yk_set_image first");
    if (c->y0 != 0 || c->h != c->fullH) return yk_refuse(c, YK_ERR_STATE, "yk_alpha_bitmaps_batch works on whole images, not on a stripe");
    const int N = c->nFrames, W = c->fullW, H = c->fullH;
    if (c->nPlanes == 4) {
        if (!c->alphaFinished) return yk_refuse(c, YK_ERR_STATE, "the alpha stage first: yk_encode_batch, or yk_alpha_reject + yk_alpha_finish");
        if (!c->B.keep || !c->B.bounds) return yk_refuse(c, YK_ERR_STATE, "the alpha stage first: yk_encode_batch, or yk_alpha_reject + yk_alpha_finish");
    }
    c->mipValid = false;
    c->mipBytes.assign((size_t)N, 0u);
    for (int f = 0; f < N; f++) {                                                          // no alpha plane: EncoderContext.cpp:1419-1426
        yk_mip_info& o = infos[f];
        o.hasChunk = 0; o.bounds[0] = 0; o.bounds[1] = 0; o.bounds[2] = W; o.bounds[3] = H;
        o.tileBBox[0] = o.tileBBox[1] = o.tileBBox[2] = o.tileBBox[3] = 0; o.nBytes = 0;
    }
    if (c->nPlanes != 4) { c->mipSlot = 0; c->mipValid = true; return YK_OK; }
    YK_HIP(c, hipSetDevice(c->device));
    const size_t slot = ((((size_t)c->mtW * c->mtH + 7) / 8) + 15) & ~(size_t)15;
    YK_HIP(c, c->mipBits.reserve(c->stream, slot * (size_t)N));
    hipLaunchKernelGGL(yk_mip_bits_batch_kernel, dim3((unsigned)((slot + YK_MIP_THREADS - 1) / YK_MIP_THREADS), (unsigned)N), dim3(YK_MIP_THREADS), 0, c->stream,
                       c->B.keep, N > 1 ? c->fs.keep : 0ull, c->B.bounds + c->boundsOff, W, H, c->mtW, c->mtH, (uint32_t)slot, c->mipBits.p);
    YK_HIP(c, hipGetLastError());
    std::vector<int32_t> bnd((size_t)N * 16);
    YK_HIP(c, hipMemcpyAsync(bnd.data(), c->B.bounds, bnd.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));                                           // the one read-back: every frame's box
    for (int f = 0; f < N; f++) {
        const int32_t* b = &bnd[(size_t)f * 16 + c->boundsOff];
        yk_mip_info& o = infos[f];
        const bool whole = b[0] == 0 && b[1] == 0 && b[2] == W && b[3] == H;               // every reject discarded (:1294, :1400-1403)
        o.hasChunk = whole ? 0 : 1;
        for (int i = 0; i < 4; i++) o.bounds[i] = b[i];
        o.tileBBox[0] = b[0] >> 4; o.tileBBox[1] = b[1] >> 4; o.tileBBox[2] = (b[2] >> 4) - (b[0] >> 4); o.tileBBox[3] = (b[3] >> 4) - (b[1] >> 4);
        if (whole || b[2] < b[0] || o.tileBBox[2] <= 0 || o.tileBBox[3] <= 0 || b[0] < 0 || b[1] < 0) continue;
        const size_t sz = ((size_t)o.tileBBox[2] * o.tileBBox[3] + 7) / 8;
        if (sz > slot) return yk_refuse(c, YK_ERR_STATE, "alpha box beyond the image");
        o.nBytes = (uint32_t)sz; c->mipBytes[(size_t)f] = (uint32_t)sz;
    }
    c->mipSlot = slot; c->mipValid = true;
    return YK_OK;
}

int yk_alpha_bitmap_device(yk_ctx* c, int frame, const uint8_t** dev, size_t* nBytes) {
    if (!c) return YK_ERR_BAD_ARG;
    if (dev) *dev = nullptr;
    if (nBytes) *nBytes = 0;
    if (!dev || !nBytes) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL result pointer");
    if (!c->mipValid) return yk_refuse(c, YK_ERR_STATE, "yk_alpha_bitmaps_batch first (the bitmaps do not outlive an encode, yk_alpha_reject, a new image or new planes)");
    if (frame < 0 || frame >= (int)c->mipBytes.size()) return yk_refuse(c, YK_ERR_BAD_ARG, "frame out of range");
    const uint32_t n = c->mipBytes[(size_t)frame];
    if (!n) return YK_OK;
    *dev = c->mipBits.p + (size_t)frame * c->mipSlot; *nBytes = n;
    return YK_OK;
}

}  // extern "C"
