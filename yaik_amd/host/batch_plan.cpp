// See batch_plan.h.  The grammar and every check below mirror the chunk loop of yaik_decode.cpp (decodeChunks); a stream that breaks one of
// them is not refused here: it becomes a fallback stream and that loop gives the verdict.
#include "batch_plan.h"
#include <cstring>
#include "yaik_format.h"

using namespace yaikfmt;

namespace yaikplan {

const int PASS_SHIFT[NUM_PASSES][2] = { {4, 4}, {4, 3}, {3, 4}, {3, 3}, {3, 2}, {2, 3}, {2, 2} };

int readHeader(const void* stream, uint32_t length, int* width, int* height, bool* rgba) {
    if (!stream || length <= sizeof(FileHeader)) return 1;
    FileHeader h; memcpy(&h, stream, sizeof h);
    if (h.tag != TAG_FILE || (h.width & 7) || (h.height & 7) || h.width == 0 || h.height == 0) return 2;
    if (width) *width = h.width;
    if (height) *height = h.height;
    if (rgba) *rgba = (h.infoMask & 1) != 0;
    return 0;
}

uint32_t bitmapBytes(int pass, int w, int h) {
    u32 bigX, bigY, bitCount;
    swizzleSize(PASS_SHIFT[pass][0], PASS_SHIFT[pass][1], bigX, bigY, bitCount);
    return (uint32_t)(((w + bigX - 1) / bigX) * ((h + bigY - 1) / bigY) * bitCount / 8);
}

bool planStream(const void* stream, uint32_t length, StreamPlan& out) {
    out = StreamPlan();
    int w = 0, h = 0;
    if (readHeader(stream, length, &w, &h, nullptr) != 0) { out.why = "header"; return false; }
#define FALLBACK(text) do { out.why = (text); return false; } while (0)
    const uint8_t* p = (const uint8_t*)stream + sizeof(FileHeader);
    const uint8_t* const end = (const uint8_t*)stream + length;
    const uint64_t maxStream = (uint64_t)w * (uint64_t)h * 3 + 4096;        // no stream of an image is longer than its pixels
    int state = 0, lastPass = -1;                                           // the single decoder's states: 1 'MIPM', 2 'ALPM', 4 'GTIL', 5 '1DTL'
    for (;;) {
        if (p + 4 > end) FALLBACK("no terminator");
        HeaderBase hb; memcpy(&hb.tag, p, 4);
        if (hb.tag == TAG_END) break;
        if (state == 5) FALLBACK("a chunk behind '1DTL'");
        if (p + sizeof(HeaderBase) > end) FALLBACK("truncated chunk header");
        memcpy(&hb, p, sizeof hb);
        const uint8_t* body = p + sizeof(HeaderBase);
        const uint8_t* endBlock = body + hb.length;
        if (endBlock > end || endBlock < body) FALLBACK("truncated chunk");
        switch (hb.tag) {
        case TAG_MIPMAP: {
            if (state != 0 || hb.length < sizeof(MipmapHeader)) FALLBACK("'MIPM' out of place");
            MipmapHeader mh; memcpy(&mh, body, sizeof mh);
            if (mh.mipmapLevel != 4) FALLBACK("'MIPM' level");
            if (mh.bbox.w <= 0 || mh.bbox.h <= 0) FALLBACK("'MIPM' box");
            const uint64_t tiles = (uint64_t)mh.bbox.w * (uint64_t)mh.bbox.h;
            if (tiles > (uint64_t)((w + 15) >> 4) * (uint64_t)((h + 15) >> 4)) FALLBACK("'MIPM' box larger than the tile grid");
            const size_t need = (size_t)((tiles + 7) / 8);
            if (body + sizeof mh + need > endBlock) FALLBACK("'MIPM' bitmap");
            out.hasMip = true; out.mipBits = body + sizeof mh; out.mipBytes = (uint32_t)need;
            out.mipBox[0] = mh.bbox.x; out.mipBox[1] = mh.bbox.y; out.mipBox[2] = mh.bbox.w; out.mipBox[3] = mh.bbox.h;
            state = 1; break;
        }
        case TAG_ALPHA: {
            if (state >= 2 || hb.length < sizeof(AlphaHeader)) FALLBACK("'ALPM' out of place");
            AlphaHeader ah; memcpy(&ah, body, sizeof ah);
            if ((uint64_t)ah.streamSize > (uint64_t)(endBlock - body - sizeof ah)) FALLBACK("'ALPM' stream");
            if (ah.streamSize == 0 || (uint64_t)ah.expectedDecompressionSize > (uint64_t)w * h) FALLBACK("'ALPM' sizes");
            const int mode = ah.parameters & 7;
            const bool masked = mode == AlphaHeader::IS_6_BIT_USEMIPMAPMASK || mode == AlphaHeader::IS_6_BIT_USEMIPMAPMASK_INVERSE;
            if (mode == 7 || mode == AlphaHeader::IS_1_BIT_USEMIPMAPMASK || (masked && state == 0)) FALLBACK("'ALPM' mode");
            const int bx = ah.bbox.x, by = ah.bbox.y, bw = ah.bbox.w, bh = ah.bbox.h;
            if (bx < 0 || by < 0 || bw <= 0 || bh <= 0 || bx >= w || by >= h || bx + bw > w || by + bh > h) FALLBACK("'ALPM' box");
            uint64_t need = 0;
            if (mode == AlphaHeader::IS_1_BIT_FULL) { if (bw & 7) FALLBACK("'ALPM' box width"); need = (uint64_t)bh * (bw >> 3); }
            else if (mode == AlphaHeader::IS_8_BIT_FULL) need = (uint64_t)bw * bh;
            else { if (bw & 3) FALLBACK("'ALPM' box width"); need = masked ? 0 : (uint64_t)bh * (bw >> 2) * 3; }
            if (ah.expectedDecompressionSize < need) FALLBACK("'ALPM' payload shorter than its box");
            out.hasAlpha = true; out.alphaMode = mode;
            out.alphaBox[0] = bx; out.alphaBox[1] = by; out.alphaBox[2] = bw; out.alphaBox[3] = bh;
            out.zAlpha = body + sizeof ah; out.zAlphaBytes = ah.streamSize; out.alphaBytes = ah.expectedDecompressionSize;
            state = 2; break;
        }
        case TAG_GRADTILE: {
            if (hb.length < sizeof(HeaderGradientTile)) FALLBACK("'GTIL' header");
            HeaderGradientTile gh; memcpy(&gh, body, sizeof gh);
            const int sx = gh.format & 7, sy = (gh.format >> 3) & 7;
            int pass = -1;
            for (int i = 0; i < NUM_PASSES; i++) if (PASS_SHIFT[i][0] == sx && PASS_SHIFT[i][1] == sy) pass = i;
            if (pass < 0) FALLBACK("'GTIL' tile shape");
            if (gh.plane != 7) FALLBACK("plane-subset 'GTIL'");
            if (pass <= lastPass) FALLBACK("'GTIL' shapes out of order or repeated");
            const uint8_t* after = body + sizeof gh;
            if ((uint64_t)gh.streamBitmapSize + gh.streamRGBSizeZStd > (uint64_t)(endBlock - after)) FALLBACK("'GTIL' streams");
            if (gh.streamBitmapSize == 0 || gh.streamRGBSizeZStd == 0) FALLBACK("'GTIL' empty ZStd frame");
            if (gh.streamRGBSizeCustomCompressor > maxStream || gh.streamRGBSizeUncompressed > maxStream) FALLBACK("'GTIL' sizes");
            GradChunk& g = out.grad[pass];
            g.present = true; g.zBitmap = after; g.zBitmapBytes = gh.streamBitmapSize; g.bitmapBytes = bitmapBytes(pass, w, h);
            g.zColor = after + gh.streamBitmapSize; g.zColorBytes = gh.streamRGBSizeZStd; g.payloadBytes = gh.streamRGBSizeCustomCompressor;
            g.rgbBytes = gh.streamRGBSizeUncompressed; g.colorCompression = gh.colorCompression;
            lastPass = pass; state = 4; break;
        }
        case TAG_TILE1D: {
            if (state < 4) break;                                           // ignored before any gradient chunk, as the single decoder does
            if (hb.length < sizeof(Header1D)) FALLBACK("'1DTL' header");
            Header1D dh; memcpy(&dh, body, sizeof dh);
            const uint8_t* zt = body + sizeof dh;
            if ((uint64_t)dh.streamTypeCnt + dh.streamPixelBit > (uint64_t)(endBlock - zt)) FALLBACK("'1DTL' streams");
            if (dh.streamTypeCnt == 0 || dh.streamPixelBit == 0) FALLBACK("'1DTL' empty ZStd frame");
            if (dh.streamTypeUncmp > maxStream || dh.streamPixelUncmp > maxStream) FALLBACK("'1DTL' sizes");
            if (dh.compressionRange == 0) { out.range0 = true; FALLBACK("'1DTL' compressionRange 0"); }
            out.has1d = true; out.zType = zt; out.zTypeBytes = dh.streamTypeCnt; out.typeBytes = dh.streamTypeUncmp;
            out.zPix = zt + dh.streamTypeCnt; out.zPixBytes = dh.streamPixelBit; out.pixBytes = dh.streamPixelUncmp;
            out.compressionRange = dh.compressionRange;
            state = 5; break;
        }
        default: FALLBACK(hb.tag == TAG_TILE3D ? "'3DTL'" : "unknown tag");
        }
        p = endBlock;
    }
#undef FALLBACK
    out.batchable = true;
    return true;
}

}  // namespace yaikplan
