// yk_gather.hip — yk_device_gather: a list of segments anywhere in device memory into one buffer, with one launch.
//
// A batch leaves what a consumer needs in several buffers of the handle (tile bitmaps, corner payloads, 1-D streams, alpha payloads), as thousands
// of segments between 0 bytes and tens of MB.  Copying them one by one costs a stream operation each; this kernel's grid follows the bytes instead:
// a workgroup of 256 lanes moves ONE piece of 4 KB of one segment, 16 bytes per lane, so a wave's load and store each cover 1 KB of contiguous
// memory.  The host uploads, per call, the exclusive prefix of the segments' piece counts and one record {source, destination offset, length} per
// segment; a workgroup finds its segment by a binary search over the prefixes (its piece number is uniform, so these are scalar loads).
// Destination offsets are multiples of 16 and so is the destination's base: every store of a whole 16 bytes is aligned.  A source that is not
// 16-byte aligned is read through a byte pointer with no alignment assumed, like the byte path of yk_unpack_u8_kernel (gfx950 allows unaligned
// global loads).  The last 1..15 bytes of a segment are moved byte by byte: nothing outside a segment is written.  No LDS, no atomics.
#include "yk_common.h"
#include <cstring>

#define YK_GA_THREADS 256
#define YK_GA_PIECE   4096          // bytes per workgroup: YK_GA_THREADS lanes x 16 bytes
#define YK_GA_MAX_SEGS 262144

namespace {
struct YkGaSeg { const uint8_t* src; unsigned long long dstOff, n; };
typedef uint32_t yk_ga4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint8_t YkGaGlobalU8;
typedef __attribute__((address_space(1))) yk_ga4 YkGaGlobal4;

__global__ __launch_bounds__(YK_GA_THREADS) void yk_gather_kernel(const uint32_t* __restrict__ prefix, const YkGaSeg* __restrict__ seg, int nSeg, uint8_t* __restrict__ dst) {
    const uint32_t p = blockIdx.x;                                   // < prefix[nSeg], the number of pieces
    int lo = 0, hi = nSeg - 1;                                       // the segment s with prefix[s] <= p < prefix[s + 1] (empty segments own no piece)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid + 1] > p) hi = mid; else lo = mid + 1;
    }
    const YkGaSeg g = seg[lo];
    const unsigned long long o = (unsigned long long)(p - prefix[lo]) * YK_GA_PIECE + threadIdx.x * 16u;
    if (o >= g.n) return;
    const YkGaGlobalU8* __restrict__ s = (const YkGaGlobalU8*)g.src + o;      // the record's pointer is generic to the compiler: global loads, not flat
    uint8_t* __restrict__ d = dst + g.dstOff + o;
    if (o + 16 <= g.n) {
        yk_ga4 v;
        if ((reinterpret_cast<uintptr_t>(g.src) & 15) == 0) v = *(const YkGaGlobal4*)s;
        else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                v[j] = (uint32_t)s[4 * j] | ((uint32_t)s[4 * j + 1] << 8) | ((uint32_t)s[4 * j + 2] << 16) | ((uint32_t)s[4 * j + 3] << 24);
        }
        *reinterpret_cast<yk_ga4*>(d) = v;
    } else {
        const int r = (int)(g.n - o);                                // the segment's last 1..15 bytes
        for (int i = 0; i < r; i++) d[i] = s[i];
    }
}
}  // namespace

extern "C" int yk_device_gather(yk_ctx* c, const void* const* devSrc, const size_t* nBytes, int nSeg, void* devDst, size_t cap, size_t* offsets, size_t* total) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!nBytes || !offsets || !total || (devDst && !devSrc)) return yk_refuse(c, YK_ERR_BAD_ARG, "devSrc, nBytes, offsets or total is NULL");
    if (nSeg < 1 || nSeg > YK_GA_MAX_SEGS) return yk_refuse(c, YK_ERR_BAD_ARG, "nSeg must be 1..262144");
    if (devDst) for (int i = 0; i < nSeg; i++) if (nBytes[i] && !devSrc[i]) return yk_refuse(c, YK_ERR_BAD_ARG, "a segment has a length and a NULL pointer");
    if (reinterpret_cast<uintptr_t>(devDst) & 15) return yk_refuse(c, YK_ERR_BAD_ARG, "devDst must be a multiple of 16");
    size_t end = 0, pieces = 0;
    for (int i = 0; i < nSeg; i++) {
        if (nBytes[i] > ((size_t)1 << 46) || end > ((size_t)1 << 62)) return yk_refuse(c, YK_ERR_BAD_ARG, "2^31 or more 4 KB pieces in one call");
        pieces += (nBytes[i] + YK_GA_PIECE - 1) / YK_GA_PIECE;
        end = (end + nBytes[i] + 15) & ~(size_t)15;
    }
    if (pieces >= ((size_t)1 << 31)) return yk_refuse(c, YK_ERR_BAD_ARG, "2^31 or more 4 KB pieces in one call");
    end = 0;
    for (int i = 0; i < nSeg; i++) { offsets[i] = end; end = (end + nBytes[i] + 15) & ~(size_t)15; }
    *total = end;
    if (!devDst) return YK_OK;                                                            // size query
    if (cap < end) return yk_refuse(c, YK_ERR_RANGE, "destination buffer too small");
    if (!pieces) return YK_OK;                                                            // nothing but empty segments
    YK_HIP(c, hipSetDevice(c->device));
    const size_t oSeg = (((size_t)nSeg + 1) * sizeof(uint32_t) + 15) & ~(size_t)15, tabBytes = oSeg + (size_t)nSeg * sizeof(YkGaSeg);
    YK_HIP(c, c->gatherTab.reserve(c->stream, tabBytes));
    int slot = 0; void* host = nullptr;
    { const int rc = yk_dec_table_host(c, tabBytes, &slot, &host); if (rc) return rc; }
    uint32_t* pre = static_cast<uint32_t*>(host);
    YkGaSeg* rec = reinterpret_cast<YkGaSeg*>(static_cast<uint8_t*>(host) + oSeg);
    uint32_t run = 0;
    for (int i = 0; i < nSeg; i++) {
        pre[i] = run; run += (uint32_t)((nBytes[i] + YK_GA_PIECE - 1) / YK_GA_PIECE);
        rec[i].src = static_cast<const uint8_t*>(devSrc[i]); rec[i].dstOff = offsets[i]; rec[i].n = nBytes[i];
    }
    pre[nSeg] = run;
    { const int rc = yk_dec_table_upload(c, slot, c->gatherTab.p, tabBytes); if (rc) return rc; }
    hipLaunchKernelGGL(yk_gather_kernel, dim3(run), dim3(YK_GA_THREADS), 0, c->stream, reinterpret_cast<const uint32_t*>(c->gatherTab.p),
                       reinterpret_cast<const YkGaSeg*>(c->gatherTab.p + oSeg), nSeg, static_cast<uint8_t*>(devDst));
    YK_HIP(c, hipGetLastError());
    return YK_OK;
}
