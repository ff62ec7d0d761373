#include "encode_frame.h"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include "chunks.h"
#include "zstd_dl.h"

namespace yaikenc {

static const int kPass[7][2] = { {4, 4}, {4, 3}, {3, 4}, {3, 3}, {3, 2}, {2, 3}, {2, 2} };      // EncoderContext.cpp:9057-9093

bool planFrame(const FramePieces& p, FrameStreams& s, std::string& err) {
    for (int i = 0; i < 7; i++) {
        s.has[i] = p.bitmap[i] && yaikchunk::gradientTileHasChunk(p.width, p.height, kPass[i][0], kPass[i][1], p.bitmap[i], p.rgbBytes[i]);
        if (!s.has[i] && p.rgbBytes[i]) { err = "a pass has colours but no tile"; return false; }   // the device coded it, the host coder would have skipped it
    }
    return true;
}

bool compressJob(const FramePieces& p, FrameStreams& s, int job, int level, std::string& err) {
    const int lv = level ? level : 18;                                       // CompressStream's level (:3697)
    if (job == 0) return p.alphaMode < 0 || yaikchunk::compressAlphaStream(p.alpha, p.alphaBytes, level, s.zAlpha, err);
    if (job <= 7) { const int i = job - 1; return !s.has[i] || yaikchunk::compressStream(p.bitmap[i], p.bitmapBytes[i], lv, s.zBitmap[i], err); }
    if (job <= 14) { const int i = job - 8; return !s.has[i] || yaikchunk::compressStream(p.palette[i], p.paletteBytes[i], lv, s.zRgb[i], err); }
    if (!p.pixBytes) return true;                                            // no '1DTL' chunk for an empty stream (:8525)
    return job == 15 ? yaikchunk::compressStream(p.pix, p.pixBytes, lv, s.zPix, err) : yaikchunk::compressStream(p.type, p.typeBytes, lv, s.zType, err);
}

bool emitFrame(const FramePieces& p, const FrameStreams& s, int colorQuad, int color1D, int range1D, std::vector<u8>& out, std::string& err) {
    char* buf = nullptr; size_t len = 0;
    FILE* f = open_memstream(&buf, &len);                                    // the chunk writers take a FILE*
    if (!f) { err = "open_memstream"; return false; }
    bool ok = yaikchunk::writeFileHeader(f, p.width, p.height, p.hasAlpha);
    if (!ok) err = "fwrite";
    if (ok && p.hasAlpha && p.mipHasChunk && !yaikchunk::writeMipmap(f, p.mipBox, 4, p.mipBits, p.mipBytes)) { ok = false; err = "fwrite"; }   // mipmapLevel = maxMipLevel + 1 (:1384)
    if (ok && p.hasAlpha && p.alphaMode >= 0) ok = yaikchunk::emitAlpha(f, p.alphaMode, p.alphaBox, p.alphaBytes, s.zAlpha, err);
    for (int i = 0; ok && i < 7; i++)
        if (s.has[i]) ok = yaikchunk::emitGradientTile(f, p.width, p.height, kPass[i][0], kPass[i][1], p.bitmap[i], p.rgbBytes[i], (u32)p.paletteBytes[i],
                                                       s.zBitmap[i], s.zRgb[i], colorQuad, 7, err);
    if (ok && p.pixBytes) ok = yaikchunk::emitTile1D(f, p.pixBytes, p.typeBytes, s.zPix, s.zType, color1D, range1D, err);
    if (ok && !yaikchunk::writeEndOfFile(f)) { ok = false; err = "fwrite"; }
    if (fclose(f) != 0 && ok) { ok = false; err = "fclose"; }
    if (ok) out.assign(reinterpret_cast<u8*>(buf), reinterpret_cast<u8*>(buf) + len);
    free(buf);
    return ok;
}

void parallelFor(size_t n, int threads, const std::function<void(size_t)>& fn) {
    std::atomic<size_t> next(0);
    auto work = [&] { for (size_t i = next++; i < n; i = next++) fn(i); };
    std::vector<std::thread> pool;
    const size_t workers = threads < 1 ? 1 : (size_t)threads, extra = n == 0 ? 0 : (workers < n ? workers : n) - 1;   // the caller is a worker too
    for (size_t t = 0; t < extra; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

bool encodeFrames(const FramePieces* frames, int n, int level, int threads, std::vector<std::vector<u8>>& out, int* failedIndex, std::string& err) {
    if (failedIndex) *failedIndex = -1;
    if (!yaikzstd::available()) { err = yaikzstd::lastError(); return false; }                  // also: the library is loaded before any worker asks for it
    out.resize((size_t)n);
    std::vector<FrameStreams> st((size_t)n);
    std::vector<std::string> errs((size_t)n);
    std::vector<char> bad((size_t)n, 0);
    parallelFor((size_t)n, threads, [&](size_t f) { if (!planFrame(frames[f], st[f], errs[f])) bad[f] = 1; });
    // the largest streams first: 1-D pixels, then 'ALPM', colour payloads, tile bitmaps, 1-D types; a frame's jobs touch different members of its
    // FrameStreams, and a failing job is the only writer of its frame's message after the plan
    static const int order[JOBS_PER_FRAME] = { 15, 0, 8, 9, 10, 11, 12, 13, 14, 1, 2, 3, 4, 5, 6, 7, 16 };
    std::vector<std::atomic<int>> failedJob((size_t)n);
    for (auto& a : failedJob) a.store(0);
    parallelFor((size_t)n * JOBS_PER_FRAME, threads, [&](size_t k) {
        const size_t f = k % (size_t)n; const int job = order[k / (size_t)n];
        if (bad[f]) return;
        std::string e;
        if (!compressJob(frames[f], st[f], job, level, e) && failedJob[f].fetch_add(1) == 0) errs[f] = e;
    });
    parallelFor((size_t)n, threads, [&](size_t f) {
        if (bad[f] || failedJob[f].load()) { bad[f] = 1; return; }
        if (!emitFrame(frames[f], st[f], 250, 255, 15, out[f], errs[f])) bad[f] = 1;              // EncoderContext's colorCompressionQuad, colorCompression1D, rangeCompression1D
    });
    for (int f = 0; f < n; f++) if (bad[(size_t)f]) {
        if (failedIndex) *failedIndex = f;
        err = "frame " + std::to_string(f) + ": " + errs[(size_t)f];
        return false;
    }
    return true;
}

}  // namespace yaikenc
