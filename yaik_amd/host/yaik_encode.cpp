// YAIK_EncodeImagesFromDevice[Alpha6]: the device's batch calls, one gather, one download, then the entropy stage of encode_frame.cpp.
#include "yaik_encode_alpha6.h"
#include <chrono>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/yaik_hip.h"
#include "alpha6_rule.h"
#include "encode_frame.h"
#include "zstd_dl.h"

struct YAIK_Encoder {
    int device = 0;
    yk_ctx* ctx = nullptr;
    std::string err;
    void* devBuf = nullptr; size_t devCap = 0;          // the gathered pieces in HBM (grow-only)
    u8* host = nullptr; size_t hostCap = 0;             // ... and on the host (grow-only)
    std::vector<std::vector<u8>> streams; bool valid = false;
    double ms[4] = { 0, 0, 0, 0 };
    // per-call tables, kept for their capacity
    std::vector<yk_frame_streams> table; std::vector<yk_mip_info> mip; std::vector<yk_alpha_info> alpha;
    std::vector<const void*> src; std::vector<size_t> len, off;
    std::vector<yaikenc::FramePieces> pieces;
    std::vector<u8> bits, force8;                       // alpha6Bit: every frame's 'MIPM' slot on the host, and the force8Bit flags the rule gives
    std::vector<const uint8_t*> bitAt;                  // ... and where the library keeps frame f's bits in HBM (NULL: none)
};

namespace {
const int SEGS_PER_FRAME = 18;                          // 'MIPM' bits, 'ALPM' payload, 7 x (tile bitmap, colour payload), 1-D types, 1-D pixels: file order

bool refuse(YAIK_ENC e, const char* what) { e->err = what; return false; }

// a device call failed: its message, and a fresh handle for the next call (a handle keeps the first message it ever failed with)
bool deviceFail(YAIK_ENC e, const char* what) {
    e->err = what;
    if (e->ctx) {
        const char* m = yk_last_error(e->ctx);
        if (m && *m) { e->err += ": "; e->err += m; }
        if (e->devBuf) { yk_device_free(e->ctx, e->devBuf); e->devBuf = nullptr; e->devCap = 0; }
        yk_destroy(e->ctx); e->ctx = nullptr;
    }
    return false;
}

double msSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

extern "C" {

YAIK_ENC YAIK_EncoderCreate(int device) {
    yk_ctx* c = nullptr;
    if (yk_create(device, &c) != YK_OK) return nullptr;
    YAIK_Encoder* e = new YAIK_Encoder();
    e->device = device; e->ctx = c;
    return e;
}

void YAIK_EncoderRelease(YAIK_ENC e) {
    if (!e) return;
    if (e->ctx) { if (e->devBuf) yk_device_free(e->ctx, e->devBuf); yk_destroy(e->ctx); }
    free(e->host);
    delete e;
}

const char* YAIK_EncoderLastError(YAIK_ENC e) { return e ? e->err.c_str() : "null encoder"; }

void YAIK_LastEncodeStageMs(YAIK_ENC e, double out[4]) { for (int i = 0; i < 4; i++) out[i] = e ? e->ms[i] : 0; }

bool YAIK_EncodedStream(YAIK_ENC e, int frame, const uint8_t** data, uint32_t* length) {
    if (data) *data = nullptr;
    if (length) *length = 0;
    if (!e || !data || !length) return false;
    if (!e->valid) return refuse(e, "no encoded streams: the last YAIK_EncodeImagesFromDevice failed, or none was made");
    if (frame < 0 || frame >= (int)e->streams.size()) return refuse(e, "frame out of range");
    *data = e->streams[(size_t)frame].data(); *length = (uint32_t)e->streams[(size_t)frame].size();
    return true;
}

}  // extern "C"

// the one body of YAIK_EncodeImagesFromDevice (alpha6Bit = 0) and YAIK_EncodeImagesFromDeviceAlpha6
static bool encodeImages(YAIK_ENC e, const uint8_t* devPixels, size_t rowBytes, size_t frameBytes, int channels, int width, int height, int n,
                         int emitAlpha, int alpha6Bit, int zstdLevel, int threads, int32_t* failedIndex) {
    if (failedIndex) *failedIndex = -1;
    if (!e) return false;
    e->valid = false; e->err.clear();
    for (double& v : e->ms) v = 0;
    if (!devPixels) return refuse(e, "devPixels is NULL");
    if (n < 1 || n > 1024) return refuse(e, "n must be 1..1024");
    if (channels != 3 && channels != 4) return refuse(e, "channels must be 3 (RGB) or 4 (RGBA)");
    if (width < 8 || height < 8 || (width & 7) || (height & 7) || width > 32760 || height > 32760) return refuse(e, "width and height must be multiples of 8 from 8 to 32760");
    if (rowBytes < (size_t)width * channels) return refuse(e, "rowBytes is shorter than a row");
    if (n > 1 && frameBytes < rowBytes * (size_t)height) return refuse(e, "frameBytes is shorter than a frame");
    if (emitAlpha != 0 && emitAlpha != 1) return refuse(e, "emitAlpha must be 0 or 1");
    if (alpha6Bit != 0 && alpha6Bit != 1) return refuse(e, "alpha6Bit must be 0 or 1");
    if (zstdLevel < 0 || zstdLevel > 22) return refuse(e, "zstdLevel must be 0 (as ConvertHotPath) or 1..22");
    if (threads < 1 || threads > 16) return refuse(e, "threads must be 1..16");
    if (!yaikzstd::available()) return refuse(e, yaikzstd::lastError());
    if (!e->ctx && yk_create(e->device, &e->ctx) != YK_OK) { e->ctx = nullptr; return refuse(e, "no usable HIP device (this path has no CPU fallback)"); }
    yk_ctx* c = e->ctx;
    const auto t0 = std::chrono::steady_clock::now();
    const bool rgba = channels == 4, wantAlpha = rgba && emitAlpha;
    // ---- the device's batch calls: a constant number of launches and read-backs, whatever n is
    if (yk_set_image(c, width, height, channels, 0, height, 0) != YK_OK) return deviceFail(e, "yk_set_image");
    if (yk_set_batch(c, n) != YK_OK) return deviceFail(e, "yk_set_batch");
    if (yk_load_device_pixels_u8(c, devPixels, rowBytes, frameBytes, channels) != YK_OK) return deviceFail(e, "yk_load_device_pixels_u8");
    if (yk_encode_batch(c, 3, 0) != YK_OK) return deviceFail(e, "yk_encode_batch");
    if (yk_encode_streams_batch(c, YK_STREAMS_CORNERS | YK_STREAMS_RANGE1D) != YK_OK) return deviceFail(e, "yk_encode_streams_batch");
    e->table.resize((size_t)n);
    if (yk_batch_streams_table(c, e->table.data()) != YK_OK) return deviceFail(e, "yk_batch_streams_table");
    if (yk_palette_compress_batch(c) != YK_OK) return deviceFail(e, "yk_palette_compress_batch");
    e->mip.assign((size_t)n, yk_mip_info{}); e->alpha.assign((size_t)n, yk_alpha_info{ -1, { 0, 0, 0, 0 }, 0 });
    if (rgba && yk_alpha_bitmaps_batch(c, e->mip.data()) != YK_OK) return deviceFail(e, "yk_alpha_bitmaps_batch");
    if (wantAlpha && !alpha6Bit && yk_alpha_values_batch(c, 1, e->alpha.data()) != YK_OK) return deviceFail(e, "yk_alpha_values_batch");
    if (wantAlpha && alpha6Bit) {
        // alpha6BitDecodable's rule per frame, on the bits of every frame in one download: the slots lie in one buffer of the handle
        // (yk_alpha_bitmaps_batch), so the span from the lowest slot to the end of the highest is fetched whole and frame f's bits are read
        // at the address the library hands out for it -- no layout is assumed beyond "one buffer"
        e->bitAt.assign((size_t)n, nullptr);
        const uint8_t* lo = nullptr; const uint8_t* hi = nullptr;
        for (int f = 0; f < n; f++) {
            const uint8_t* d = nullptr; size_t nb = 0;
            if (yk_alpha_bitmap_device(c, f, &d, &nb) != YK_OK) return deviceFail(e, "yk_alpha_bitmap_device");
            if (!d || nb != e->mip[(size_t)f].nBytes) continue;
            e->bitAt[(size_t)f] = d;
            if (!lo || d < lo) lo = d;
            if (!hi || d + nb > hi) hi = d + nb;
        }
        e->bits.resize(lo ? (size_t)(hi - lo) : 0);
        if (lo && yk_device_download(c, e->bits.data(), lo, e->bits.size()) != YK_OK) return deviceFail(e, "yk_device_download");
        e->force8.assign((size_t)n, 1);
        for (int f = 0; f < n; f++) {
            const yk_mip_info& m = e->mip[(size_t)f];
            if (e->bitAt[(size_t)f] && yaikalpha6::decodable(m.hasChunk != 0, m.tileBBox, e->bits.data() + (e->bitAt[(size_t)f] - lo), m.nBytes)) e->force8[(size_t)f] = 0;
        }
        if (yk_alpha_values_mask_batch(c, e->force8.data(), e->alpha.data()) != YK_OK) return deviceFail(e, "yk_alpha_values_mask_batch");
    }
    // ---- the segment list: every frame's pieces in file order
    const size_t nSeg = (size_t)n * SEGS_PER_FRAME;
    e->src.assign(nSeg, nullptr); e->len.assign(nSeg, 0); e->off.assign(nSeg, 0);
    for (int f = 0; f < n; f++) {
        const void** s = &e->src[(size_t)f * SEGS_PER_FRAME]; size_t* l = &e->len[(size_t)f * SEGS_PER_FRAME];
        const yk_frame_streams& t = e->table[(size_t)f];
        const uint8_t* d = nullptr; size_t nb = 0;
        if (rgba) { if (yk_alpha_bitmap_device(c, f, &d, &nb) != YK_OK) return deviceFail(e, "yk_alpha_bitmap_device"); s[0] = d; l[0] = nb; }
        if (wantAlpha) { if (yk_alpha_payload_device(c, f, &d, &nb) != YK_OK) return deviceFail(e, "yk_alpha_payload_device"); s[1] = d; l[1] = nb; }
        for (int p = 0; p < 7; p++) {
            s[2 + 2 * p] = t.bitmap[p]; l[2 + 2 * p] = t.bitmap[p] ? t.bitmapBytes[p] : 0;
            if (yk_palette_payload_device(c, f * 7 + p, &d, &nb) != YK_OK) return deviceFail(e, "yk_palette_payload_device");
            s[3 + 2 * p] = d; l[3 + 2 * p] = nb;
        }
        s[16] = t.type; l[16] = t.typeBytes; s[17] = t.pix; l[17] = t.pixBytes;
    }
    const auto t1 = std::chrono::steady_clock::now();
    // ---- one gather, one download
    size_t total = 0;
    if (yk_device_gather(c, e->src.data(), e->len.data(), (int)nSeg, nullptr, 0, e->off.data(), &total) != YK_OK) return deviceFail(e, "yk_device_gather");
    if (total > e->devCap) {
        if (e->devBuf) { yk_device_free(c, e->devBuf); e->devBuf = nullptr; e->devCap = 0; }
        if (yk_device_alloc(c, total, &e->devBuf) != YK_OK) { e->devBuf = nullptr; return deviceFail(e, "yk_device_alloc"); }
        e->devCap = total;
    }
    if (total > e->hostCap) {
        free(e->host); e->hostCap = 0;
        e->host = static_cast<u8*>(malloc(total));
        if (!e->host) return refuse(e, "out of host memory");
        e->hostCap = total;
    }
    if (total && yk_device_gather(c, e->src.data(), e->len.data(), (int)nSeg, e->devBuf, e->devCap, e->off.data(), &total) != YK_OK) return deviceFail(e, "yk_device_gather");
    if (yk_device_download(c, e->host, e->devBuf, total) != YK_OK) return deviceFail(e, "yk_device_download");     // synchronises: the pixels have been read
    const auto t2 = std::chrono::steady_clock::now();
    // ---- entropy stage and framing on the workers
    e->pieces.assign((size_t)n, yaikenc::FramePieces());
    for (int f = 0; f < n; f++) {
        yaikenc::FramePieces& p = e->pieces[(size_t)f];
        const size_t* o = &e->off[(size_t)f * SEGS_PER_FRAME]; const size_t* l = &e->len[(size_t)f * SEGS_PER_FRAME];
        const yk_mip_info& m = e->mip[(size_t)f]; const yk_alpha_info& a = e->alpha[(size_t)f];
        p.width = width; p.height = height; p.hasAlpha = rgba;
        p.mipHasChunk = rgba && m.hasChunk != 0;
        for (int k = 0; k < 4; k++) { p.mipBox[k] = m.tileBBox[k]; p.alphaBox[k] = a.bbox[k]; }
        p.mipBits = e->host + o[0]; p.mipBytes = l[0];
        p.alphaMode = wantAlpha ? a.mode : -1; p.alpha = e->host + o[1]; p.alphaBytes = l[1];
        for (int k = 0; k < 7; k++) {
            p.bitmap[k] = l[2 + 2 * k] ? e->host + o[2 + 2 * k] : nullptr; p.bitmapBytes[k] = l[2 + 2 * k];
            p.rgbBytes[k] = e->table[(size_t)f].rgbBytes[k];
            p.palette[k] = e->host + o[3 + 2 * k]; p.paletteBytes[k] = l[3 + 2 * k];
        }
        p.type = e->host + o[16]; p.typeBytes = l[16]; p.pix = e->host + o[17]; p.pixBytes = l[17];
    }
    int failed = -1;
    const bool ok = yaikenc::encodeFrames(e->pieces.data(), n, zstdLevel, threads, e->streams, &failed, e->err);
    e->ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    e->ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
    e->ms[2] = msSince(t2); e->ms[3] = msSince(t0);
    if (!ok) { if (failedIndex) *failedIndex = failed; return false; }
    for (const auto& s : e->streams) if (s.size() > 0xFFFFFFFFu) return refuse(e, "a stream of 4 GB or more");
    e->valid = true;
    return true;
}

extern "C" {

bool YAIK_EncodeImagesFromDevice(YAIK_ENC e, const uint8_t* devPixels, size_t rowBytes, size_t frameBytes, int channels, int width, int height, int n,
                                 int emitAlpha, int zstdLevel, int threads, int32_t* failedIndex) {
    return encodeImages(e, devPixels, rowBytes, frameBytes, channels, width, height, n, emitAlpha, 0, zstdLevel, threads, failedIndex);
}

bool YAIK_EncodeImagesFromDeviceAlpha6(YAIK_ENC e, const uint8_t* devPixels, size_t rowBytes, size_t frameBytes, int channels, int width, int height,
                                       int n, int emitAlpha, int alpha6Bit, int zstdLevel, int threads, int32_t* failedIndex) {
    return encodeImages(e, devPixels, rowBytes, frameBytes, channels, width, height, n, emitAlpha, alpha6Bit, zstdLevel, threads, failedIndex);
}

}  // extern "C"
