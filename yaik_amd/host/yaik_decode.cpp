// See yaik_decode.h.  Control flow mirrors decoder/YAIK_API.cpp (Init :86-131, Pre :441-497, DecodeImage :600-1342): slot
// stack, first-error-wins sticky code, chunk state machine, "Pre must be followed by Decode".  The per-pixel work is done by
// the HIP kernels behind yk_decode_*; ZStd runs on the host like in the reference, and so does PaletteDecompressor unless
// YAIK_SetDevicePalette(1) sends the 'GTIL' payloads of whole-RGB chunks to yk_decode_gradient_palette.
#include "yaik_decode.h"
#include "yaik_decode_window.h"
#include "yaik_decode_multiwindow.h"
#include "yaik_decode_batch_windows.h"
#include "yaik_decode_window_px.h"
#include "../csrc/yk_window_px.h"
#include "../csrc/yk_window_mirror.h"
#include "yaik_decode_norm.h"
#include "../csrc/yk_resample.h"
#include "yaik_decode_resample.h"
#include "yaik_decode_scaled.h"
#include "yaik_decode_mipchain.h"
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include "../../include/yaik_hip.h"
#include "batch_plan.h"
#include "palette.h"
#include "yaik_format.h"
#include "zstd_dl.h"

using namespace yaikfmt;

namespace {
std::atomic<int> gError{YAIK_NO_ERROR};
void setError(YAIK_ERROR_CODE e) { int expected = YAIK_NO_ERROR; gError.compare_exchange_strong(expected, (int)e); }   // first error wins (:77-84)

struct Slot {
    yk_ctx* ctx = nullptr;
    void* srcCheck = nullptr; uint32_t srcLength = 0;
    int width = 0, height = 0; bool isRGBA = false;
    std::vector<uint8_t> stage; void* devStage = nullptr; size_t devStageCap = 0;   // YAIK_DecodeImagesToDevice: grow-only staging, host and HBM
};
struct Library {
    std::vector<Slot> slots;
    std::vector<Slot*> freeStack;
    std::mutex lock;                                    // the reference's stack is unguarded although Pre/Decode are documented thread-safe
    YAIK_SMemAlloc alloc;
    bool hasLut = false;                                // YAIK_AssignLUT handed a valid 3-D LUT file to every decode slot
};
Library* gLib = nullptr;
int gDevice = 0;

void* defaultAlloc(void*, size_t n) { return malloc(n); }
void  defaultFree(void*, void* p) { free(p); }

void defaultImageBuilder(YAIK_SDecodedImage*, YAIK_SCustomDataSource*) {}      // marker: the de-tile kernel writes outputImage directly

bool zexpand(const uint8_t* src, uint32_t n, uint32_t expected, std::vector<uint8_t>& out, size_t slack) {
    out.assign((size_t)expected + slack, 0);
    if (n == 0) return false;                                                   // DecompressData returns NULL for an empty stream (:517-519)
    if (!yaikzstd::decompress(out.data(), expected, src, n)) { setError(YAIK_INVALID_DECOMPRESSION); return false; }
    return true;
}
}

void YAIK_SetDevice(int device) { gDevice = device; }
static int gConsistentMarks = 0;
void YAIK_SetPartialPlaneMarks(int consistent) { gConsistentMarks = consistent ? 1 : 0; }
static int gDevicePalette = 0;
void YAIK_SetDevicePalette(int on) { gDevicePalette = on ? 1 : 0; }

YAIK_LIB YAIK_Init(uint8_t maxDecodeThreadContext, YAIK_SMemAlloc* libraryMemAllocator) {
    if (maxDecodeThreadContext == 0) { setError(YAIK_INVALID_CONTEXT_COUNT); return nullptr; }
    if (gLib) { setError(YAIK_INIT_FAIL); return nullptr; }                     // one library per process, like the reference's gLibrary
    if (!yaikzstd::available()) { setError(YAIK_DECOMPRESSION_CREATE_FAIL); return nullptr; }
    Library* L = new Library();
    if (libraryMemAllocator) {
        if (!libraryMemAllocator->customAlloc || !libraryMemAllocator->customFree) { delete L; setError(YAIK_INVALID_CONTEXT_MEMALLOCATOR); return nullptr; }
        L->alloc = *libraryMemAllocator;
    }
    L->slots.resize(maxDecodeThreadContext);
    for (auto& s : L->slots) {
        if (yk_create(gDevice, &s.ctx) != YK_OK) {                              // no HIP device: refuse, there is no CPU decode path here
            for (auto& t : L->slots) if (t.ctx) yk_destroy(t.ctx);
            delete L; setError(YAIK_INIT_FAIL); return nullptr;
        }
        L->freeStack.push_back(&s);
    }
    gLib = L;
    return L;
}

// decoder/YAIK_API.cpp:133-415: only the 3-D table file ('LUL') is accepted ('LU2' is deprecated there too); the per-orientation tables are
// laid out in HBM by every decode slot's handle (yk_decode_assign_lut)
void YAIK_AssignLUT(YAIK_LIB lib, uint8_t* lutData, uint32_t lutDataLength) {
    if (!lib || lib != gLib) { setError(YAIK_INVALID_LIBRARYCTX); return; }
    if (!lutData || lutDataLength < sizeof(LUTHeader) || lutData[0] != 'L' || lutData[1] != 'U' || lutData[2] != 'L') { setError(YAIK_INVALID_LUT); return; }
    const uint32_t expected = ((uint32_t)lutData[5] + 1) * 3 * (64 + 32 + 16 + 8);
    if (expected != lutDataLength - sizeof(LUTHeader)) { setError(YAIK_INVALID_LUT); return; }
    for (auto& s : gLib->slots)
        if (yk_decode_assign_lut(s.ctx, lutData, lutDataLength) != YK_OK) { setError(YAIK_MALLOC_FAIL); return; }
    gLib->hasLut = true;
}

void YAIK_Release(YAIK_LIB lib) {
    if (!lib || lib != gLib) { setError(YAIK_RELEASE_EMPTY_LIBRARY); return; }
    for (auto& s : gLib->slots) if (s.ctx) { if (s.devStage) yk_device_free(s.ctx, s.devStage); yk_destroy(s.ctx); }
    delete gLib; gLib = nullptr;
}

YAIK_ERROR_CODE YAIK_GetErrorCode() { return (YAIK_ERROR_CODE)gError.exchange(YAIK_NO_ERROR); }

bool YAIK_DecodeImagePre(YAIK_LIB lib, void* stream, uint32_t length, YAIK_SDecodedImage* info) {
    if (!info) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
    info->hasAlpha = false; info->hasAlpha1Bit = false; info->outputImage = nullptr; info->width = 0; info->height = 0; info->internalTag = nullptr;
    if (!lib || lib != gLib) { setError(YAIK_INVALID_LIBRARYCTX); return false; }
    const FileHeader* h = (const FileHeader*)stream;
    if (!h || length <= sizeof(FileHeader)) { setError(YAIK_INVALID_STREAM); return false; }
    if (h->tag != TAG_FILE || (h->width & 7) || (h->height & 7) || h->width == 0 || h->height == 0) { setError(YAIK_INVALID_HEADER); return false; }
    Slot* s = nullptr;
    { std::lock_guard<std::mutex> g(gLib->lock); if (!gLib->freeStack.empty()) { s = gLib->freeStack.back(); gLib->freeStack.pop_back(); } }
    if (!s) { setError(YAIK_NO_EMPTYDECODE_SLOT); return false; }
    s->srcCheck = stream; s->srcLength = length; s->width = h->width; s->height = h->height; s->isRGBA = (h->infoMask & 1) != 0;
    info->width = h->width; info->height = h->height; info->hasAlpha = s->isRGBA; info->internalTag = s;
    info->customImageOutput = defaultImageBuilder; info->userContextCustomImage = nullptr;
    info->userMemoryAllocator.customAlloc = defaultAlloc; info->userMemoryAllocator.customFree = defaultFree; info->userMemoryAllocator.customContext = nullptr;
    return true;
}

// The chunk state machine shared by YAIK_DecodeImage, YAIK_DecodeImageToDevice and the fallback of YAIK_DecodeImagesToDevice: begins a single
// image on the slot's handle and runs every chunk up to the terminator; hasAlphaPlane = an 'ALPM' chunk was decoded (pCtx->alphaChannel).
// window = {x0, y0, ww, wh} (YAIK_DecodeImageWindowToDevice): set on the handle right after the begin, so every chunk may skip what lies outside it
static bool decodeChunks(Slot* s, const void* stream, uint32_t length, bool& hasAlphaPlane, const int* window = nullptr, bool px = false) {
    std::vector<uint8_t> bitmap, pal, rgb, types, pix;
    hasAlphaPlane = false;
    {
        const int w = s->width, h = s->height;
        if (yk_decode_begin(s->ctx, w, h) != YK_OK) { setError(YAIK_MALLOC_FAIL); return false; }
        if (window && (px ? yk_decode_set_window_px(s->ctx, window[0], window[1], window[2], window[3])
                          : yk_decode_set_window(s->ctx, window[0], window[1], window[2], window[3])) != YK_OK) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
        const uint8_t* p = (const uint8_t*)stream + sizeof(FileHeader);
        const uint8_t* const end = (const uint8_t*)stream + length;
        int state = 0; bool bad = false;
        std::vector<uint8_t> mask, alphaRaw; size_t maskBytes = 0; int32_t maskBox[4] = { 0, 0, 0, 0 };
        while (!bad) {
            if (p + 4 > end) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
            HeaderBase hb; memcpy(&hb.tag, p, 4);
            if (hb.tag == TAG_END) break;
            if (p + sizeof(HeaderBase) > end) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
            memcpy(&hb, p, sizeof hb);
            const uint8_t* body = p + sizeof(HeaderBase);
            const uint8_t* endBlock = body + hb.length;
            if (endBlock > end || endBlock < body) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }     // never read past the stream (:724-728)
            switch (hb.tag) {
            case TAG_MIPMAP: {
                if (state != 0 || hb.length < sizeof(MipmapHeader)) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                MipmapHeader mh; memcpy(&mh, body, sizeof mh);
                if (mh.mipmapLevel != 4) { setError(YAIK_INVALID_MIPMAP_LEVEL); bad = true; break; }         // only level 4 is implemented (YAIK_Mipmap.cpp:53-54)
                const size_t need = ((size_t)mh.bbox.w * mh.bbox.h + 7) / 8;
                if (mh.bbox.w <= 0 || mh.bbox.h <= 0 || body + sizeof mh + need > endBlock) { setError(YAIK_INVALID_STREAM); bad = true; break; }
                mask.assign((size_t)((w + 15) >> 4) * ((h + 15) >> 4) * 32 + 64, 0);                            // the tile grid, clipped edge tiles included
                if (yk_decode_mask(s->ctx, body + sizeof mh, mh.bbox.w, mh.bbox.h, mask.data(), mask.size()) != YK_OK) { setError(YAIK_INVALID_STREAM); bad = true; break; }
                maskBytes = (size_t)mh.bbox.w * mh.bbox.h * 32;                                             // pCtx->mipMapMask, box in pixels (YAIK_Mipmap.cpp:35-39)
                maskBox[0] = mh.bbox.x << 4; maskBox[1] = mh.bbox.y << 4; maskBox[2] = mh.bbox.w << 4; maskBox[3] = mh.bbox.h << 4;
                state = 1; break;
            }
            case TAG_GRADTILE: {
                if (state > 4) break;                                                                       // silently skipped after '1DTL' (:836)
                if (hb.length < sizeof(HeaderGradientTile)) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                state = 4;
                HeaderGradientTile gh; memcpy(&gh, body, sizeof gh);
                const int sx = gh.format & 7, sy = (gh.format >> 3) & 7;
                u32 bigX, bigY, bitCount;
                if (!swizzleSize(sx, sy, bigX, bigY, bitCount) || gh.plane < 1 || gh.plane > 7) { setError(YAIK_INVALID_PLANE_ID); bad = true; break; }
                const uint8_t* after = body + sizeof gh;
                if (after + (size_t)gh.streamBitmapSize + gh.streamRGBSizeZStd > endBlock) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                const uint32_t sizeBitmap = (uint32_t)(((w + bigX - 1) / bigX) * ((h + bigY - 1) / bigY) * bitCount / 8);
                if (!zexpand(after, gh.streamBitmapSize, sizeBitmap, bitmap, 0)) { bad = true; break; }
                if (!zexpand(after + gh.streamBitmapSize, gh.streamRGBSizeZStd, gh.streamRGBSizeCustomCompressor, pal, 128 * 3)) { bad = true; break; }
                if (gDevicePalette && gh.plane == 7 && gh.streamRGBSizeUncompressed % 3 == 0) {
                    // YAIK_SetDevicePalette(1): the payload goes to the device as it is; PaletteDecompressor, its status check and the pass run there
                    if (yk_decode_gradient_palette(s->ctx, sx, sy, bitmap.data(), sizeBitmap, pal.data(), gh.streamRGBSizeCustomCompressor,
                                                   gh.streamRGBSizeUncompressed, gh.colorCompression) != YK_OK) { setError(YAIK_INVALID_STREAM); bad = true; }
                    break;
                }
                const size_t slack = (size_t)((w + 3) >> 2) * ((h + 3) >> 2) * 12;                          // the reference's "secure buffer" (:901)
                rgb.assign((size_t)gh.streamRGBSizeUncompressed + slack, 0);
                if (!PaletteDecompressor(pal.data(), (int)gh.streamRGBSizeCustomCompressor, (int)gh.streamRGBSizeCustomCompressor + 128 * 3, rgb.data(),
                                         (int)gh.streamRGBSizeUncompressed, gh.colorCompression)) { setError(YAIK_INVALID_STREAM); bad = true; break; }
                if (gh.plane != 7) {
                    // a chunk for one or two planes splits the masks per plane first (UpdateTileAndRGBMask, YAIK_API.cpp:876-878); only the 4x4
                    // decoders exist for such chunks, every other tile shape returns without touching anything (YAIK_Gradient.cpp:29-36)
                    if (yk_decode_split_masks(s->ctx) != YK_OK) { setError(YAIK_INVALID_STREAM); bad = true; break; }
                    if (sx == 2 && sy == 2 && yk_decode_gradient_planes(s->ctx, gh.plane, gConsistentMarks, bitmap.data(), sizeBitmap, rgb.data(),
                                                                       gh.streamRGBSizeUncompressed) != YK_OK) { setError(YAIK_INVALID_STREAM); bad = true; }
                    break;
                }
                if (yk_decode_gradient(s->ctx, sx, sy, bitmap.data(), sizeBitmap, rgb.data(), gh.streamRGBSizeUncompressed) != YK_OK) { setError(YAIK_INVALID_STREAM); bad = true; }
                break;
            }
            case TAG_TILE1D: {
                if (state < 4) break;                                                                       // ignored before any gradient chunk (:962)
                if (hb.length < sizeof(Header1D)) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                state = 5;
                Header1D dh; memcpy(&dh, body, sizeof dh);
                const uint8_t* zt = body + sizeof dh; const uint8_t* zp = zt + dh.streamTypeCnt;
                if (zp + dh.streamPixelBit > endBlock) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                if (!zexpand(zt, dh.streamTypeCnt, dh.streamTypeUncmp, types, 64) || !zexpand(zp, dh.streamPixelBit, dh.streamPixelUncmp, pix, 64)) { bad = true; break; }
                if (yk_decode_1d(s->ctx, types.data(), dh.streamTypeUncmp, pix.data(), dh.streamPixelUncmp, dh.compressionRange) != YK_OK) { setError(YAIK_INVALID_STREAM); bad = true; }
                break;
            }
            case TAG_ALPHA: {                                                                              // decoder/YAIK_API.cpp:750-833
                if (state >= 2) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }                      // only before any 'GTIL' (:753-756)
                if (hb.length < sizeof(AlphaHeader)) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                AlphaHeader ah; memcpy(&ah, body, sizeof ah);
                if ((uint64_t)ah.streamSize > (uint64_t)(endBlock - body - sizeof ah)) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                // a payload is at most one byte per pixel: nothing is expanded for a larger claim
                if (ah.streamSize == 0 || (uint64_t)ah.expectedDecompressionSize > (uint64_t)w * h) { setError(YAIK_INVALID_STREAM); bad = true; break; }
                if (!zexpand(body + sizeof ah, ah.streamSize, ah.expectedDecompressionSize, alphaRaw, 0)) { bad = true; break; }   // DecompressData (:759)
                const int mode = ah.parameters & 7;
                if (mode == 7) { setError(YAIK_INVALID_ALPHA_FORMAT); bad = true; break; }
                if (state == 0 && (mode == AlphaHeader::IS_1_BIT_USEMIPMAPMASK || mode == AlphaHeader::IS_6_BIT_USEMIPMAPMASK ||
                                   mode == AlphaHeader::IS_6_BIT_USEMIPMAPMASK_INVERSE)) { setError(YAIK_ALPHA_FORMAT_IMPOSSIBLE); bad = true; break; }   // :779-785
                if (mode == AlphaHeader::IS_1_BIT_USEMIPMAPMASK) { setError(YAIK_ALPHA_UNSUPPORTED_YET); bad = true; break; }   // state 1 (:799-801)
                const bool masked = mode == AlphaHeader::IS_6_BIT_USEMIPMAPMASK || mode == AlphaHeader::IS_6_BIT_USEMIPMAPMASK_INVERSE;
                const int32_t bb[4] = { ah.bbox.x, ah.bbox.y, ah.bbox.w, ah.bbox.h };
                // 1-bit rows as the encoder writes them (refQuirk 0: the reference's own loop drops a byte per row)
                if (yk_decode_alpha(s->ctx, mode, bb, alphaRaw.data(), ah.expectedDecompressionSize, masked ? mask.data() : nullptr, masked ? maskBytes : 0,
                                    masked ? maskBox : nullptr, 0) != YK_OK) { setError(YAIK_INVALID_STREAM); bad = true; break; }
                hasAlphaPlane = true;
                state = 2;
                break;
            }
            case TAG_TILE3D: {                                                                             // decoder/YAIK_API.cpp:999-1300
                if (state > 4) break;
                state = 4;
                if (hb.length < sizeof(HeaderTile3D)) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                if (!gLib->hasLut) { setError(YAIK_INVALID_LUT); bad = true; break; }                       // the reference would read a NULL table here
                HeaderTile3D th; memcpy(&th, body, sizeof th);
                // The counts come from an untrusted stream: all size arithmetic in 64 bits, and nothing is expanded before the counts are
                // plausible (a tile is at least 4x4 pixels; six colour bytes per tile; the reference leaves both checks a TODO, :1079).
                const uint64_t maxTiles = (uint64_t)(w / 4) * (uint64_t)(h / 4);
                if ((uint64_t)th.streamTypeCnt > maxTiles || (uint64_t)th.streamColorCnt != 6ull * (uint64_t)th.streamTypeCnt) { setError(YAIK_INVALID_STREAM); bad = true; break; }
                const uint8_t* q = body + sizeof th;
                const uint32_t cmp[12] = { th.compr3BitSize, th.compr4BitSize, th.compr5BitSize, th.compr6BitSize, th.comprTypeSize, th.comprColorSize,
                                           th.sizeT16_8MapCmp, th.sizeT8_16MapCmp, th.sizeT8_8MapCmp, th.sizeT8_4MapCmp, th.sizeT4_8MapCmp, th.sizeT4_4MapCmp };
                const uint32_t raw[12] = { th.stream3BitCnt, th.stream4BitCnt, th.stream5BitCnt, th.stream6BitCnt, th.streamTypeCnt * 2, th.streamColorCnt,
                                           th.sizeT16_8Map, th.sizeT8_16Map, th.sizeT8_8Map, th.sizeT8_4Map, th.sizeT4_8Map, th.sizeT4_4Map };
                std::vector<uint8_t> part[12];
                const uint64_t maxStream = (uint64_t)w * (uint64_t)h * 3 + 4096;                            // no stream of an image can be longer than its pixels
                for (int k = 0; k < 12 && !bad; k++) if ((uint64_t)raw[k] > maxStream) { setError(YAIK_INVALID_STREAM); bad = true; }
                for (int k = 0; k < 12 && !bad; k++) {
                    if ((uint64_t)cmp[k] > (uint64_t)(endBlock - q)) { setError(YAIK_INVALID_TAG_ID); bad = true; break; }
                    if (raw[k] && !zexpand(q, cmp[k], raw[k], part[k], 256)) { bad = true; break; }
                    q += cmp[k];
                }
                if (bad) break;
                // what yk_decode_lut3d may read is what was really expanded, not what the header claims
                if (part[4].size() < (size_t)th.streamTypeCnt * 2 || part[5].size() < (size_t)th.streamTypeCnt * 6) { setError(YAIK_INVALID_STREAM); bad = true; break; }
                if (th.streamColorCnt) PaletteFullRangeRemapping(part[5].data(), (int)th.streamColorCnt, th.compressionRateColor);
                const uint8_t* maps[6]; size_t mapBytes[6]; const uint8_t* idx[4]; size_t idxBytes[4]; size_t used[6];
                for (int k = 0; k < 6; k++) { maps[k] = raw[6 + k] ? part[6 + k].data() : nullptr; mapBytes[k] = raw[6 + k]; }
                for (int k = 0; k < 4; k++) { idx[k] = raw[k] ? part[k].data() : nullptr; idxBytes[k] = raw[k]; }
                if (yk_decode_lut3d(s->ctx, maps, mapBytes, reinterpret_cast<const uint16_t*>(part[4].data()), th.streamTypeCnt, part[5].data(), idx, idxBytes, used) != YK_OK) {
                    setError(YAIK_INVALID_STREAM); bad = true;
                }
                break;
            }
            default: setError(YAIK_INVALID_TAG_ID); bad = true; break;
            }
            p = endBlock;
        }
        return !bad;
    }
}

// YAIK_DecodeImage, YAIK_DecodeImageToDevice and YAIK_DecodeImageWindowToDevice; toDevice: outputImage is in device memory (default builder only);
// window (with toDevice): only that rectangle is decoded and written; level (with toDevice, YAIK_DecodeImageScaledToDevice): the output is the
// image at 1 / (1 << level) size; mip (with toDevice, YAIK_DecodeImageMipchainToDevice): the outputs are the levels of a mip chain, outputImage is unused
namespace { struct MipRequest { int first, n; void* const* images; const uint32_t* strides; }; }
static bool decodeImage(void* stream, uint32_t length, YAIK_SDecodedImage* info, bool toDevice, const int* window = nullptr, int level = 0, const MipRequest* mip = nullptr,
                        bool px = false) {
    if (!info || !info->internalTag || !gLib) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
    Slot* s = (Slot*)info->internalTag;
    bool res = false;
    const YAIK_SMemAlloc& ua = info->userMemoryAllocator;
    const bool customBuilder = info->customImageOutput && info->customImageOutput != defaultImageBuilder;
    do {
        if (toDevice && customBuilder) { setError(YAIK_DECIMG_INVALIDCTX); break; }               // a custom builder takes host planes
        if (level < 0 || level > 3) { setError(YAIK_DECIMG_INVALIDCTX); break; }                  // before any chunk is decoded or a byte written
        if (!ua.customAlloc || !ua.customFree) { setError(YAIK_INVALID_CONTEXT_MEMALLOCATOR); break; }
        if (s->srcCheck != stream || s->srcLength != length) { setError(YAIK_DECIMG_DIFFSTREAM); break; }
        if (!mip && !info->outputImage) { setError(YAIK_DECIMG_BUFFERNOTSET); break; }
        const int w = s->width, h = s->height;
        bool hasAlphaPlane = false;
        if (mip) {                                                                                  // range and pointers before any chunk is decoded
            const int total = yk_decode_mip_levels(w, h);
            bool ok = mip->first >= 0 && mip->n >= 1 && mip->n <= YK_MIP_MAX_LEVELS && mip->first <= total - mip->n && mip->images && mip->strides;
            for (int i = 0; ok && i < mip->n; i++) ok = mip->images[i] != nullptr;
            if (!ok) { setError(YAIK_DECIMG_INVALIDCTX); break; }
        }
        if (window && px && !yk_wpx_window_ok(window[0], window[1], window[2], window[3], w, h)) { setError(YAIK_DECIMG_INVALIDCTX); break; }   // a pixel window: any rectangle inside the image
        if (window && !px && (((window[0] | window[1] | window[2] | window[3]) & 7) || window[0] < 0 || window[1] < 0 || window[2] < 8 || window[3] < 8 ||
                       window[0] > w - window[2] || window[1] > h - window[3])) { setError(YAIK_DECIMG_INVALIDCTX); break; }
        if (!decodeChunks(s, stream, length, hasAlphaPlane, window, px)) break;
        if (customBuilder) {
            // custom builder: hand over the 8x8-tiled planes exactly like the reference (:1303-1318)
            const size_t planeSize = (size_t)(w / 8) * (h / 8) * 64;
            uint8_t* planes = (uint8_t*)ua.customAlloc(ua.customContext, planeSize * 3);
            if (!planes) { setError(YAIK_MALLOC_FAIL); break; }
            if (yk_decode_planes(s->ctx, planes, planes + planeSize, planes + 2 * planeSize, planeSize) == YK_OK) {
                YAIK_SCustomDataSource src;
                src.planeR = planes; src.planeG = planes + planeSize; src.planeB = planes + 2 * planeSize; src.planeA = nullptr;
                std::vector<uint8_t> alphaHost;
                if (hasAlphaPlane) {                                                                    // linear alpha, strideA = w (:1306-1310)
                    alphaHost.resize((size_t)w * h);
                    if (yk_decode_alpha_plane(s->ctx, alphaHost.data(), alphaHost.size()) != YK_OK) { setError(YAIK_INVALID_STREAM); ua.customFree(ua.customContext, planes); break; }
                    src.planeA = alphaHost.data();
                }
                src.strideR = src.strideG = src.strideB = (w / 8) * 64; src.strideA = w;
                info->customImageOutput(info, &src);
                res = true;
            } else setError(YAIK_INVALID_STREAM);
            ua.customFree(ua.customContext, planes);
        } else {
            // default builder = the de-tile kernel.  Without an 'ALPM' chunk, like the reference's pCtx->alphaChannel the alpha plane is
            // NULL and internal_imageBuilderFunc takes its RGB branch (3 B/pixel) whether or not the header says RGBA (YAIK_API.cpp:1316,
            // YAIK_DefaultCallback.cpp:44,63); row padding is left untouched.
            // with an 'ALPM' chunk: RGBA 4 B/pixel from the alpha plane kept in HBM (YAIK.h documents RGBA rows; the reference's own RGBA
            // branch is defective)
            if (mip) {
                yk_mip_level lv[YK_MIP_MAX_LEVELS];
                for (int i = 0; i < mip->n; i++) lv[i] = { (uint8_t*)mip->images[i], (size_t)mip->strides[i], 0, 0 };
                res = yk_decode_output_mipchain_device(s->ctx, mip->first, mip->n, lv, hasAlphaPlane ? 4 : 3, -1) == YK_OK && yk_synchronize(s->ctx) == YK_OK;
            } else if (toDevice)                                                                    // the same kernel into device rows, then a fence:
                res = info->outputImageStride > 0 &&
                      (level  ? yk_decode_output_scaled_device(s->ctx, level, info->outputImage, (size_t)info->outputImageStride, 0, hasAlphaPlane ? 4 : 3, -1)
                       : window ? yk_decode_output_window_device(s->ctx, info->outputImage, (size_t)info->outputImageStride, 0, hasAlphaPlane ? 4 : 3, -1)
                              : yk_decode_output_device(s->ctx, info->outputImage, (size_t)info->outputImageStride, 0, hasAlphaPlane ? 4 : 3, -1)) == YK_OK &&
                      yk_synchronize(s->ctx) == YK_OK;                                              // the slot's stream is idle before it is released
            else
                res = (hasAlphaPlane ? yk_decode_output_alpha(s->ctx, info->outputImage, (size_t)info->outputImageStride)
                                     : yk_decode_output(s->ctx, info->outputImage, (size_t)info->outputImageStride, nullptr, w)) == YK_OK;
            if (!res) setError(YAIK_INVALID_STREAM);
        }
    } while (false);
    { std::lock_guard<std::mutex> g(gLib->lock); gLib->freeStack.push_back(s); }     // the slot is released whatever happened (:1322-1337)
    info->internalTag = nullptr;
    return res;
}

bool YAIK_DecodeImage(void* stream, uint32_t length, YAIK_SDecodedImage* info) { return decodeImage(stream, length, info, false); }
bool YAIK_DecodeImageToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info) { return decodeImage(stream, length, info, true); }
extern "C" bool YAIK_DecodeImageWindowToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info, int x0, int y0, int ww, int wh) {
    const int window[4] = { x0, y0, ww, wh };
    return decodeImage(stream, length, info, true, window);
}
// yaik_decode_window_px.h
extern "C" bool YAIK_DecodeImageWindowPxToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info, int x0, int y0, int ww, int wh) {
    const int window[4] = { x0, y0, ww, wh };
    return decodeImage(stream, length, info, true, window, 0, nullptr, true);
}
extern "C" bool YAIK_DecodeImageScaledToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info, int level) {
    return decodeImage(stream, length, info, true, nullptr, level);
}
extern "C" bool YAIK_DecodeImageMipchainToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info, int firstLevel, int nLevels, void* const* levelImages,
                                                 const uint32_t* levelStrides) {
    const MipRequest mip = { firstLevel, nLevels, levelImages, levelStrides };
    return decodeImage(stream, length, info, true, nullptr, 0, &mip);
}

// ---- YAIK_DecodeImagesToDevice: n streams of one shape through the device's batch calls (yaik_decode.h) ------------------------------------
namespace {
int gBatchFallbacks = 0;
double gBatchMs[3] = { 0, 0, 0 };

size_t place(size_t& total, size_t bytes) { const size_t at = total; total = (total + bytes + 15) & ~(size_t)15; return at; }

// where the pieces of one batchable stream lie in the staging buffer
struct FrameStage {
    size_t bitmap[yaikplan::NUM_PASSES] = {}, color[yaikplan::NUM_PASSES] = {}, type = 0, pix = 0, alpha = 0, mip = 0;
};

double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}

int  YAIK_LastBatchFallbacks() { return gBatchFallbacks; }
void YAIK_LastBatchStageMs(double out[3]) { if (out) for (int i = 0; i < 3; i++) out[i] = gBatchMs[i]; }

// YAIK_DecodeImagesToDevice and, with xy (one origin per stream) and the window size ww x wh, YAIK_DecodeImagesWindowsToDevice: the same plan,
// expansion, upload and batch calls; with windows the batch is given them right after yk_decode_begin_batch, the output is the windows' and a
// fallback stream takes the single-image window chain; with norm (YAIK_DecodeImagesNormToDevice, yaik_decode_norm.h) both end in the normalised outputs:
// devOut holds elements of norm->dtype, the pitches stay in bytes, mirror is NULL or one flag per stream; with ow > 0
// (YAIK_DecodeImagesResampledToDevice, yaik_decode_resample.h) the batch gets rsRects (NULL: whole frames) through yk_decode_set_batch_rects and both
// end in the resampled outputs of ow x oh, uint8 if norm is NULL; a fallback stream decodes its rectangle as a pixel window
static bool decodeImages(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, uint8_t* devOut, size_t rowBytes, size_t planeBytes,
                         size_t frameBytes, int channels, int threads, int32_t* failedIndex, const int* xy, int ww, int wh, bool px = false, const yk_norm* norm = nullptr,
                         const uint8_t* mirror = nullptr, const int* rsRects = nullptr, int ow = 0, int oh = 0) {
    using namespace yaikplan;
    if (failedIndex) *failedIndex = -1;
    if (!lib || lib != gLib) { setError(YAIK_INVALID_LIBRARYCTX); return false; }
    if (!streams || !lengths || n < 1 || n > 1024 || (channels != 3 && channels != 4) || threads < 1 || threads > 16) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
    if (!devOut) { setError(YAIK_DECIMG_BUFFERNOTSET); return false; }
    if (norm) {                                                                 // the device call's own rule, before a slot is taken
        bool ok = norm->dtype == YK_ELEM_F16 || norm->dtype == YK_ELEM_BF16 || norm->dtype == YK_ELEM_F32;
        for (int k = 0; ok && k < 4; k++) ok = yk_norm_param_ok(norm->scale[k]) && yk_norm_param_ok(norm->bias[k]);
        const size_t es = norm->dtype == YK_ELEM_F32 ? 4 : 2;
        if (!ok || (((uintptr_t)devOut | rowBytes | planeBytes | frameBytes) & (es - 1))) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
    }
    // the headers: the checks of YAIK_DecodeImagePre on every stream, then one shape
    int w = 0, h = 0;
    for (int f = 0; f < n; f++) {
        int fw = 0, fh = 0;
        const int rc = readHeader(streams[f], lengths[f], &fw, &fh, nullptr);
        if (rc == 0 && f == 0) { w = fw; h = fh; }
        if (rc != 0 || fw != w || fh != h) { setError(rc == 1 ? YAIK_INVALID_STREAM : YAIK_INVALID_HEADER); if (failedIndex) *failedIndex = f; return false; }
    }
    const bool rs = ow > 0;
    if (rs) {                                                                   // the rule of yk_resample.h for every stream, before a slot is taken
        bool ok = yk_rs_size_ok(ow, oh) && (rsRects || yk_rs_src_ok(0, 0, w, h, w, h));
        for (int f = 0; ok && rsRects && f < n; f++) ok = yk_rs_src_ok(rsRects[4 * f], rsRects[4 * f + 1], rsRects[4 * f + 2], rsRects[4 * f + 3], w, h);
        if (!ok) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
    }
    if (xy && px) {                                                             // pixel windows: any rectangle inside the image
        if (!yk_wpx_windows_ok(n, xy, ww, wh, w, h)) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
    } else if (xy) {                                                            // the rule of yk_decode_set_window for every stream, before a slot is taken or a byte written
        bool ok = !((ww | wh) & 7) && ww >= 8 && wh >= 8 && ww <= w && wh <= h;
        for (int f = 0; ok && f < n; f++) ok = !((xy[2 * f] | xy[2 * f + 1]) & 7) && xy[2 * f] >= 0 && xy[2 * f + 1] >= 0 && xy[2 * f] <= w - ww && xy[2 * f + 1] <= h - wh;
        if (!ok) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
    }
    Slot* s = nullptr;
    { std::lock_guard<std::mutex> g(gLib->lock); if (!gLib->freeStack.empty()) { s = gLib->freeStack.back(); gLib->freeStack.pop_back(); } }
    if (!s) { setError(YAIK_NO_EMPTYDECODE_SLOT); return false; }
    s->width = w; s->height = h;
    bool res = false;
    int failed = -1;
    gBatchFallbacks = 0;
    do {
        const double t0 = nowMs();
        // ---- plan: sizes come from the chunk headers, so every region of the staging buffer is known before anything is expanded
        std::vector<StreamPlan> plan((size_t)n);
        std::vector<char> fallback((size_t)n, 0);
        for (int f = 0; f < n; f++) fallback[(size_t)f] = planStream(streams[f], lengths[f], plan[(size_t)f]) ? 0 : 1;
        // a '1DTL' chunk with compressionRange 0 is refused by the single-image chain whatever else the stream holds: the call fails here, before
        // a byte of devOut is written
        for (int f = 0; f < n && failed < 0; f++) if (plan[(size_t)f].range0) failed = f;
        if (failed >= 0) { setError(YAIK_INVALID_STREAM); break; }
        int range1d = 0, colorCompression = -1;
        bool devicePalette = gDevicePalette != 0, anyAlpha = false, any1d = false;
        for (int f = 0; f < n; f++) {
            if (fallback[(size_t)f]) continue;
            const StreamPlan& P = plan[(size_t)f];
            if (P.has1d) { if (!range1d) range1d = P.compressionRange; else if (P.compressionRange != range1d) { fallback[(size_t)f] = 1; continue; } }
            for (int p = 0; p < NUM_PASSES; p++) {
                const GradChunk& g = P.grad[p];
                if (!g.present) continue;
                if (colorCompression < 0) colorCompression = g.colorCompression;
                if (g.colorCompression != colorCompression || g.rgbBytes % 3 || (g.rgbBytes && !g.payloadBytes)) devicePalette = false;
            }
        }
        size_t total = 0;
        size_t zeroBitmap[NUM_PASSES], bmBytes[NUM_PASSES];
        for (int p = 0; p < NUM_PASSES; p++) { bmBytes[p] = bitmapBytes(p, w, h); zeroBitmap[p] = place(total, bmBytes[p]); }
        std::vector<FrameStage> at((size_t)n);
        for (int f = 0; f < n; f++) {
            if (fallback[(size_t)f]) continue;
            const StreamPlan& P = plan[(size_t)f]; FrameStage& A = at[(size_t)f];
            for (int p = 0; p < NUM_PASSES; p++) if (P.grad[p].present) {
                A.bitmap[p] = place(total, bmBytes[p]);
                // host coder: the colour stream with PaletteDecompressor's slack behind it; device coder: the payload as ZStd left it
                A.color[p] = place(total, devicePalette ? (size_t)P.grad[p].payloadBytes + 16 : (size_t)P.grad[p].rgbBytes + 16);
            }
            if (P.has1d) { A.type = place(total, (size_t)P.typeBytes + 64); A.pix = place(total, (size_t)P.pixBytes + 64); any1d = true; }
            if (P.hasAlpha) { A.alpha = place(total, P.alphaBytes); anyAlpha = true; }
            if (P.hasMip) A.mip = place(total, P.mipBytes);
        }
        if (s->stage.size() < total) s->stage.resize(total);
        uint8_t* const S = s->stage.data();
        for (int p = 0; p < NUM_PASSES; p++) memset(S + zeroBitmap[p], 0, bmBytes[p]);
        // ---- expand: ZStd (and the host's PaletteDecompressor) on the workers, one stream per task; a stream that fails becomes a fallback stream
        std::atomic<int> next{0};
        const bool devPal = devicePalette;
        auto work = [&]() {
            std::vector<uint8_t> pal;
            for (int f; (f = next.fetch_add(1)) < n;) {
                if (fallback[(size_t)f]) continue;
                const StreamPlan& P = plan[(size_t)f]; const FrameStage& A = at[(size_t)f];
                bool ok = true;
                for (int p = 0; p < NUM_PASSES && ok; p++) {
                    const GradChunk& g = P.grad[p];
                    if (!g.present) continue;
                    ok = yaikzstd::decompress(S + A.bitmap[p], g.bitmapBytes, g.zBitmap, g.zBitmapBytes);
                    if (!ok) break;
                    if (devPal) { ok = yaikzstd::decompress(S + A.color[p], g.payloadBytes, g.zColor, g.zColorBytes); continue; }
                    pal.assign((size_t)g.payloadBytes + 128 * 3, 0);
                    ok = yaikzstd::decompress(pal.data(), g.payloadBytes, g.zColor, g.zColorBytes);
                    if (!ok) break;
                    // PaletteDecompressor writes whole tokens: into a buffer with the single decoder's slack, then the stream itself is kept
                    std::vector<uint8_t> rgb((size_t)g.rgbBytes + (size_t)((w + 3) >> 2) * ((h + 3) >> 2) * 12, 0);
                    ok = PaletteDecompressor(pal.data(), (int)g.payloadBytes, (int)g.payloadBytes + 128 * 3, rgb.data(), (int)g.rgbBytes, g.colorCompression);
                    if (ok) memcpy(S + A.color[p], rgb.data(), g.rgbBytes);
                }
                if (ok && P.has1d) ok = yaikzstd::decompress(S + A.type, P.typeBytes, P.zType, P.zTypeBytes) && yaikzstd::decompress(S + A.pix, P.pixBytes, P.zPix, P.zPixBytes);
                if (ok && P.hasAlpha) ok = yaikzstd::decompress(S + A.alpha, P.alphaBytes, P.zAlpha, P.zAlphaBytes);
                if (ok && P.hasMip) memcpy(S + A.mip, P.mipBits, P.mipBytes);
                if (!ok) fallback[(size_t)f] = 1;
            }
        };
        {
            const int nt = threads < n ? threads : n;
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(work);
            work();
            for (auto& t : pool) t.join();
        }
        const double t1 = nowMs();
        // ---- upload: one copy
        if (s->devStageCap < total) {
            if (s->devStage) { yk_device_free(s->ctx, s->devStage); s->devStage = nullptr; s->devStageCap = 0; }
            if (yk_device_alloc(s->ctx, total, &s->devStage) != YK_OK) { setError(YAIK_MALLOC_FAIL); break; }
            s->devStageCap = total;
        }
        const uint8_t* const D = (const uint8_t*)s->devStage;
        if (yk_device_upload(s->ctx, s->devStage, S, total) != YK_OK) { setError(YAIK_MALLOC_FAIL); break; }
        const double t2 = nowMs();
        // ---- decode: every kernel once over the n frames; a fallback stream is an empty frame here
        if (yk_decode_begin_batch(s->ctx, w, h, n) != YK_OK) { setError(YAIK_MALLOC_FAIL); break; }
        if (xy && (px ? yk_decode_set_batch_windows_px(s->ctx, xy, ww, wh) : yk_decode_set_batch_windows(s->ctx, xy, ww, wh)) != YK_OK) { setError(YAIK_DECIMG_INVALIDCTX); break; }
        if (rs && rsRects && yk_decode_set_batch_rects(s->ctx, rsRects) != YK_OK) { setError(YAIK_DECIMG_INVALIDCTX); break; }
        const size_t NP = (size_t)n * NUM_PASSES;
        std::vector<const uint8_t*> bm(NP), rgb(NP, nullptr);
        std::vector<size_t> rgbBytes(NP, 0);
        for (int f = 0; f < n; f++)
            for (int p = 0; p < NUM_PASSES; p++) {
                const bool has = !fallback[(size_t)f] && plan[(size_t)f].grad[p].present;
                bm[(size_t)f * NUM_PASSES + p] = D + (has ? at[(size_t)f].bitmap[p] : zeroBitmap[p]);
                if (has && plan[(size_t)f].grad[p].rgbBytes) { rgb[(size_t)f * NUM_PASSES + p] = D + at[(size_t)f].color[p]; rgbBytes[(size_t)f * NUM_PASSES + p] = plan[(size_t)f].grad[p].rgbBytes; }
            }
        bool bad = false;
        if (devicePalette) {
            // the payloads went up as they are: PaletteDecompressor over all of them in one call, its status checked before the gradient launch
            std::vector<const uint8_t*> pay; std::vector<size_t> payBytes, outBytes; std::vector<size_t> where;
            for (size_t i = 0; i < NP; i++) if (rgbBytes[i]) {
                pay.push_back(rgb[i]); payBytes.push_back(plan[i / NUM_PASSES].grad[i % NUM_PASSES].payloadBytes); outBytes.push_back(rgbBytes[i]); where.push_back(i);
            }
            if (!pay.empty()) {
                std::vector<int32_t> st(pay.size());
                if (pay.size() > 65536 || yk_palette_decompress_streams(s->ctx, pay.data(), payBytes.data(), outBytes.data(), (int)pay.size(), colorCompression > 0 ? colorCompression : 1) != YK_OK ||
                    yk_palette_decode_status(s->ctx, st.data()) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
                for (size_t k = 0; k < where.size(); k++) {
                    const uint8_t* dev = nullptr; size_t nb = 0;
                    if (yk_palette_decoded_device(s->ctx, (int)k, &dev, &nb) != YK_OK) { bad = true; break; }
                    rgb[where[k]] = dev; rgbBytes[where[k]] = nb;
                    if (st[k]) fallback[where[k] / NUM_PASSES] = 1;                  // a payload the coder rejects: the single chain reports it
                }
            }
        }
        if (bad) { setError(YAIK_INVALID_STREAM); break; }
        int sx[NUM_PASSES], sy[NUM_PASSES];
        for (int p = 0; p < NUM_PASSES; p++) { sx[p] = PASS_SHIFT[p][0]; sy[p] = PASS_SHIFT[p][1]; }
        if (yk_decode_gradient_all_batch_device(s->ctx, NUM_PASSES, sx, sy, bm.data(), bmBytes, rgb.data(), rgbBytes.data(), 0) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
        {
            std::vector<const uint8_t*> ty((size_t)n, nullptr), px((size_t)n, nullptr);
            std::vector<size_t> tyB((size_t)n, 0), pxB((size_t)n, 0);
            for (int f = 0; f < n; f++) if (!fallback[(size_t)f] && plan[(size_t)f].has1d) {
                const StreamPlan& P = plan[(size_t)f];
                if (P.typeBytes) { ty[(size_t)f] = D + at[(size_t)f].type; tyB[(size_t)f] = P.typeBytes; }
                if (P.pixBytes) { px[(size_t)f] = D + at[(size_t)f].pix; pxB[(size_t)f] = P.pixBytes; }
            }
            if (yk_decode_1d_batch_device(s->ctx, ty.data(), tyB.data(), px.data(), pxB.data(), any1d && range1d ? range1d : 1) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
        }
        if (anyAlpha) {                                                        // with three channels too: its status is part of the verdict
            std::vector<int32_t> modes((size_t)n, -1), boxes((size_t)n * 4, 0), mipBoxes((size_t)n * 4, 0), st((size_t)n, 0);
            std::vector<const uint8_t*> pay((size_t)n, nullptr), bits((size_t)n, nullptr);
            std::vector<size_t> payB((size_t)n, 0), bitsB((size_t)n, 0);
            for (int f = 0; f < n; f++) if (!fallback[(size_t)f] && plan[(size_t)f].hasAlpha) {
                const StreamPlan& P = plan[(size_t)f];
                modes[(size_t)f] = P.alphaMode; pay[(size_t)f] = D + at[(size_t)f].alpha; payB[(size_t)f] = P.alphaBytes;
                for (int k = 0; k < 4; k++) boxes[(size_t)f * 4 + k] = P.alphaBox[k];
                if (P.hasMip) { bits[(size_t)f] = D + at[(size_t)f].mip; bitsB[(size_t)f] = P.mipBytes; for (int k = 0; k < 4; k++) mipBoxes[(size_t)f * 4 + k] = P.mipBox[k]; }
            }
            if (yk_decode_alpha_mask_batch_device(s->ctx, modes.data(), boxes.data(), pay.data(), payB.data(), bits.data(), bitsB.data(), mipBoxes.data(), 255) != YK_OK ||
                yk_decode_alpha_batch_status(s->ctx, st.data()) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
            for (int f = 0; f < n; f++) if (st[(size_t)f]) fallback[(size_t)f] = 1;       // a payload shorter than the mask selects: the single chain reports it
        }
        if (rs) {
            if (yk_decode_output_resampled_batch_device(s->ctx, norm, mirror, devOut, ow, oh, rowBytes, planeBytes, frameBytes, channels, anyAlpha && channels == 4 ? -1 : 255) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
        } else if (norm) {
            if (yk_decode_output_norm_batch_device(s->ctx, norm, mirror, devOut, rowBytes, planeBytes, frameBytes, channels, anyAlpha && channels == 4 ? -1 : 255) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
        } else if (xy) {
            if (yk_decode_output_batch_windows_device(s->ctx, devOut, rowBytes, planeBytes, frameBytes, channels, anyAlpha && channels == 4 ? -1 : 255) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
        } else if (anyAlpha && channels == 4) {
            if (yk_decode_output_batch_alpha_device(s->ctx, devOut, rowBytes, planeBytes, frameBytes) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
        } else if (yk_decode_output_batch_device(s->ctx, devOut, rowBytes, planeBytes, frameBytes, channels, 255) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
        if (yk_synchronize(s->ctx) != YK_OK) { setError(YAIK_INVALID_STREAM); break; }
        const double t3 = nowMs();
        gBatchMs[0] = t1 - t0; gBatchMs[1] = t2 - t1; gBatchMs[2] = t3 - t2;
        // ---- fallback: the single-image chain on the same slot, into the frame's slice of devOut
        res = true;
        for (int f = 0; f < n && res; f++) {
            if (!fallback[(size_t)f]) continue;
            gBatchFallbacks++;
            bool hasAlphaPlane = false;
            const int window[4] = { rsRects ? rsRects[4 * f] : xy ? xy[2 * f] : 0, rsRects ? rsRects[4 * f + 1] : xy ? xy[2 * f + 1] : 0, rsRects ? rsRects[4 * f + 2] : ww,
                                    rsRects ? rsRects[4 * f + 3] : wh };
            res = decodeChunks(s, streams[f], lengths[f], hasAlphaPlane, xy || rsRects ? window : nullptr, px || rsRects);
            if (res) {
                const bool plane = hasAlphaPlane && channels == 4;
                uint8_t* const dst = devOut + (size_t)f * frameBytes;
                res = (rs ? yk_decode_output_resampled_device(s->ctx, nullptr, norm, mirror ? mirror[f] : 0, dst, ow, oh, rowBytes, planeBytes, channels, plane ? -1 : 255)
                       : norm ? yk_decode_output_norm_device(s->ctx, norm, mirror ? mirror[f] : 0, dst, rowBytes, planeBytes, channels, plane ? -1 : 255)
                       : xy ? yk_decode_output_window_device(s->ctx, dst, rowBytes, planeBytes, channels, plane ? -1 : 255)
                          : yk_decode_output_device(s->ctx, dst, rowBytes, planeBytes, channels, plane ? -1 : 255)) == YK_OK && yk_synchronize(s->ctx) == YK_OK;
                if (!res) setError(YAIK_INVALID_STREAM);
            }
            if (!res) failed = f;
        }
    } while (false);
    { std::lock_guard<std::mutex> g(gLib->lock); gLib->freeStack.push_back(s); }
    if (failedIndex) *failedIndex = failed;
    return res;
}

bool YAIK_DecodeImagesToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, uint8_t* devOut, size_t rowBytes, size_t planeBytes,
                               size_t frameBytes, int channels, int threads, int32_t* failedIndex) {
    return decodeImages(lib, streams, lengths, n, devOut, rowBytes, planeBytes, frameBytes, channels, threads, failedIndex, nullptr, 0, 0);
}
// yaik_decode_batch_windows.h
extern "C" bool YAIK_DecodeImagesWindowsToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, uint8_t* devOut, size_t rowBytes, size_t planeBytes,
                                                 size_t frameBytes, int channels, int threads, int32_t* failedIndex, const int* xy, int ww, int wh) {
    if (!xy) { if (failedIndex) *failedIndex = -1; setError(YAIK_DECIMG_INVALIDCTX); return false; }
    return decodeImages(lib, streams, lengths, n, devOut, rowBytes, planeBytes, frameBytes, channels, threads, failedIndex, xy, ww, wh);
}

// yaik_decode_window_px.h
extern "C" bool YAIK_DecodeImagesWindowsPxToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, uint8_t* devOut, size_t rowBytes, size_t planeBytes,
                                                   size_t frameBytes, int channels, int threads, int32_t* failedIndex, const int* xy, int ww, int wh) {
    if (!xy) { if (failedIndex) *failedIndex = -1; setError(YAIK_DECIMG_INVALIDCTX); return false; }
    return decodeImages(lib, streams, lengths, n, devOut, rowBytes, planeBytes, frameBytes, channels, threads, failedIndex, xy, ww, wh, true);
}

// yaik_decode_norm.h
extern "C" bool YAIK_DecodeImagesNormToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, void* devOut, size_t rowBytes, size_t planeBytes,
                                              size_t frameBytes, int channels, int threads, int32_t* failedIndex, const int* xy, int ww, int wh, const yk_norm* norm,
                                              const uint8_t* mirror) {
    if (!norm) { if (failedIndex) *failedIndex = -1; setError(YAIK_DECIMG_INVALIDCTX); return false; }
    return decodeImages(lib, streams, lengths, n, static_cast<uint8_t*>(devOut), rowBytes, planeBytes, frameBytes, channels, threads, failedIndex, xy, ww, wh, true, norm, mirror);
}

// yaik_decode_resample.h
extern "C" bool YAIK_DecodeImagesResampledToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, void* devOut, size_t rowBytes, size_t planeBytes,
                                                   size_t frameBytes, int channels, int threads, int32_t* failedIndex, const int* rects, int ow, int oh, const yk_norm* norm,
                                                   const uint8_t* mirror) {
    if (ow < 1 || oh < 1) { if (failedIndex) *failedIndex = -1; setError(YAIK_DECIMG_INVALIDCTX); return false; }
    return decodeImages(lib, streams, lengths, n, static_cast<uint8_t*>(devOut), rowBytes, planeBytes, frameBytes, channels, threads, failedIndex, nullptr, 0, 0, false, norm, mirror,
                        rects, ow, oh);
}

// ---- YAIK_DecodeImageWindowsToDevice: many windows of one stream (yaik_decode_multiwindow.h) ------------------------------------------------
namespace { int gWindowsPrepared = 0; }
extern "C" int YAIK_LastWindowsPrepared(void) { return gWindowsPrepared; }

// the prepared path for a batchable stream: expand into the slot's staging buffer, one upload, prepare, alpha, one render call
static bool decodeWindowsPrepared(Slot* s, const yaikplan::StreamPlan& P, uint8_t* devOut, size_t rowBytes, int nWindows, const int* xy, int ww, int wh, size_t windowBytes,
                                  bool px) {
    using namespace yaikplan;
    const int w = s->width, h = s->height;
    size_t total = 0;
    FrameStage A;
    size_t bmBytes[NUM_PASSES];
    for (int p = 0; p < NUM_PASSES; p++) {
        bmBytes[p] = bitmapBytes(p, w, h);
        if (P.grad[p].present) { A.bitmap[p] = place(total, bmBytes[p]); A.color[p] = place(total, (size_t)P.grad[p].rgbBytes + 16); }
    }
    if (P.has1d) { A.type = place(total, (size_t)P.typeBytes + 64); A.pix = place(total, (size_t)P.pixBytes + 64); }
    if (P.hasAlpha) A.alpha = place(total, P.alphaBytes);
    if (s->stage.size() < total + 16) s->stage.resize(total + 16);
    uint8_t* const S = s->stage.data();
    std::vector<uint8_t> pal, rgb;
    for (int p = 0; p < NUM_PASSES; p++) {
        const GradChunk& g = P.grad[p];
        if (!g.present) continue;
        if (!yaikzstd::decompress(S + A.bitmap[p], g.bitmapBytes, g.zBitmap, g.zBitmapBytes)) { setError(YAIK_INVALID_DECOMPRESSION); return false; }
        pal.assign((size_t)g.payloadBytes + 128 * 3, 0);
        if (!yaikzstd::decompress(pal.data(), g.payloadBytes, g.zColor, g.zColorBytes)) { setError(YAIK_INVALID_DECOMPRESSION); return false; }
        rgb.assign((size_t)g.rgbBytes + (size_t)((w + 3) >> 2) * ((h + 3) >> 2) * 12, 0);              // PaletteDecompressor writes whole tokens: the single decoder's slack
        if (!PaletteDecompressor(pal.data(), (int)g.payloadBytes, (int)g.payloadBytes + 128 * 3, rgb.data(), (int)g.rgbBytes, g.colorCompression)) { setError(YAIK_INVALID_STREAM); return false; }
        memcpy(S + A.color[p], rgb.data(), g.rgbBytes);
    }
    if (P.has1d && !(yaikzstd::decompress(S + A.type, P.typeBytes, P.zType, P.zTypeBytes) && yaikzstd::decompress(S + A.pix, P.pixBytes, P.zPix, P.zPixBytes))) {
        setError(YAIK_INVALID_DECOMPRESSION); return false;
    }
    if (P.hasAlpha && !yaikzstd::decompress(S + A.alpha, P.alphaBytes, P.zAlpha, P.zAlphaBytes)) { setError(YAIK_INVALID_DECOMPRESSION); return false; }
    if (s->devStageCap < total + 16) {
        if (s->devStage) { yk_device_free(s->ctx, s->devStage); s->devStage = nullptr; s->devStageCap = 0; }
        if (yk_device_alloc(s->ctx, total + 16, &s->devStage) != YK_OK) { setError(YAIK_MALLOC_FAIL); return false; }
        s->devStageCap = total + 16;
    }
    const uint8_t* const D = (const uint8_t*)s->devStage;
    if (total && yk_device_upload(s->ctx, s->devStage, S, total) != YK_OK) { setError(YAIK_MALLOC_FAIL); return false; }
    if (yk_decode_begin(s->ctx, w, h) != YK_OK) { setError(YAIK_MALLOC_FAIL); return false; }
    // 'MIPM' and 'ALPM' as the single chain runs them: the mask on the host, the plane left in HBM
    std::vector<uint8_t> mask; size_t maskBytes = 0; int32_t maskBox[4] = { 0, 0, 0, 0 };
    if (P.hasMip) {
        mask.assign((size_t)((w + 15) >> 4) * ((h + 15) >> 4) * 32 + 64, 0);
        if (yk_decode_mask(s->ctx, P.mipBits, P.mipBox[2], P.mipBox[3], mask.data(), mask.size()) != YK_OK) { setError(YAIK_INVALID_STREAM); return false; }
        maskBytes = (size_t)P.mipBox[2] * P.mipBox[3] * 32;
        for (int k = 0; k < 4; k++) maskBox[k] = P.mipBox[k] << 4;
    }
    if (P.hasAlpha) {
        const bool masked = P.alphaMode == AlphaHeader::IS_6_BIT_USEMIPMAPMASK || P.alphaMode == AlphaHeader::IS_6_BIT_USEMIPMAPMASK_INVERSE;
        if (yk_decode_alpha(s->ctx, P.alphaMode, P.alphaBox, S + A.alpha, P.alphaBytes, masked ? mask.data() : nullptr, masked ? maskBytes : 0,
                            masked ? maskBox : nullptr, 0) != YK_OK) { setError(YAIK_INVALID_STREAM); return false; }
    }
    int sx[NUM_PASSES], sy[NUM_PASSES], n = 0;
    const uint8_t* bm[NUM_PASSES]; const uint8_t* col[NUM_PASSES]; size_t bmB[NUM_PASSES], colB[NUM_PASSES];
    for (int p = 0; p < NUM_PASSES; p++) {
        if (!P.grad[p].present) continue;
        sx[n] = PASS_SHIFT[p][0]; sy[n] = PASS_SHIFT[p][1];
        bm[n] = D + A.bitmap[p]; bmB[n] = bmBytes[p];
        colB[n] = P.grad[p].rgbBytes; col[n] = colB[n] ? D + A.color[p] : nullptr;
        n++;
    }
    if (yk_decode_prepare_device(s->ctx, n, sx, sy, bm, bmB, col, colB, 0, P.has1d ? D + A.type : nullptr, P.has1d ? P.typeBytes : 0,
                                 P.has1d ? D + A.pix : nullptr, P.has1d ? P.pixBytes : 0, P.has1d ? P.compressionRange : 0) != YK_OK) { setError(YAIK_INVALID_STREAM); return false; }
    if ((px ? yk_decode_render_windows_px_device(s->ctx, nWindows, xy, ww, wh, devOut, rowBytes, 0, windowBytes, P.hasAlpha ? 4 : 3, -1)
            : yk_decode_render_windows_device(s->ctx, nWindows, xy, ww, wh, devOut, rowBytes, 0, windowBytes, P.hasAlpha ? 4 : 3, -1)) != YK_OK ||
        yk_synchronize(s->ctx) != YK_OK) { setError(YAIK_INVALID_STREAM); return false; }
    return true;
}

// YAIK_DecodeImageWindowsToDevice and, with px, YAIK_DecodeImageWindowsPxToDevice (yaik_decode_window_px.h): the same chain under the other rule
static bool decodeImageWindows(void* stream, uint32_t length, YAIK_SDecodedImage* info, int nWindows, const int* xy, int ww, int wh, size_t windowBytes, bool px) {
    if (!info || !info->internalTag || !gLib) { setError(YAIK_DECIMG_INVALIDCTX); return false; }
    Slot* s = (Slot*)info->internalTag;
    bool res = false;
    gWindowsPrepared = 0;
    do {
        if (info->customImageOutput && info->customImageOutput != defaultImageBuilder) { setError(YAIK_DECIMG_INVALIDCTX); break; }   // a custom builder takes host planes
        if (!info->userMemoryAllocator.customAlloc || !info->userMemoryAllocator.customFree) { setError(YAIK_INVALID_CONTEXT_MEMALLOCATOR); break; }
        if (s->srcCheck != stream || s->srcLength != length) { setError(YAIK_DECIMG_DIFFSTREAM); break; }
        if (!info->outputImage) { setError(YAIK_DECIMG_BUFFERNOTSET); break; }
        const int w = s->width, h = s->height;
        bool ok = nWindows >= 1 && nWindows <= 1024 && xy && (px || !((ww | wh) & 7)) && ww >= (px ? 1 : 8) && wh >= (px ? 1 : 8) && ww <= w && wh <= h &&
                  info->outputImageStride > 0 && (nWindows == 1 || windowBytes / (size_t)wh >= (size_t)info->outputImageStride);
        for (int k = 0; ok && k < nWindows; k++)
            ok = (px || !((xy[2 * k] | xy[2 * k + 1]) & 7)) && xy[2 * k] >= 0 && xy[2 * k + 1] >= 0 && xy[2 * k] <= w - ww && xy[2 * k + 1] <= h - wh;
        if (!ok) { setError(YAIK_DECIMG_INVALIDCTX); break; }
        const size_t rowBytes = (size_t)info->outputImageStride;
        yaikplan::StreamPlan P;
        if (yaikplan::planStream(stream, length, P)) {
            // a 1-D chunk with one empty stream decodes to zeros in the single chain; prepare takes both lengths or none
            if (P.has1d && (!P.typeBytes || !P.pixBytes)) P.has1d = false;
            gWindowsPrepared = 1;
            res = decodeWindowsPrepared(s, P, info->outputImage, rowBytes, nWindows, xy, ww, wh, windowBytes, px);
            break;
        }
        res = true;
        for (int k = 0; k < nWindows && res; k++) {                                                   // the single-window chain, window after window
            const int window[4] = { xy[2 * k], xy[2 * k + 1], ww, wh };
            bool hasAlphaPlane = false;
            res = decodeChunks(s, stream, length, hasAlphaPlane, window, px);
            if (res) {
                res = yk_decode_output_window_device(s->ctx, info->outputImage + (size_t)k * windowBytes, rowBytes, 0, hasAlphaPlane ? 4 : 3, -1) == YK_OK &&
                      yk_synchronize(s->ctx) == YK_OK;
                if (!res) setError(YAIK_INVALID_STREAM);
            }
        }
    } while (false);
    { std::lock_guard<std::mutex> g(gLib->lock); gLib->freeStack.push_back(s); }
    info->internalTag = nullptr;
    return res;
}
extern "C" bool YAIK_DecodeImageWindowsToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info, int nWindows, const int* xy, int ww, int wh, size_t windowBytes) {
    return decodeImageWindows(stream, length, info, nWindows, xy, ww, wh, windowBytes, false);
}
extern "C" bool YAIK_DecodeImageWindowsPxToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info, int nWindows, const int* xy, int ww, int wh, size_t windowBytes) {
    return decodeImageWindows(stream, length, info, nWindows, xy, ww, wh, windowBytes, true);
}
