// CPU-only companion of YAIK_EncodeImagesFromDevice (no HIP linked): the entropy stage and framing of encode_frame.cpp on named blob files, for
// the `not gpu` tests.
//   encode_frame_tool encode <level 0..22> <threads 1..16> <out prefix> <pieces 0.blobs> [<pieces 1.blobs> ...]
//        the frames as ONE batch through yaikenc::encodeFrames; frame i goes to <out prefix><i>.yaik
//   encode_frame_tool parse <file.yaik> <out.blobs>
//        the chunk list of a stream: per chunk its tag, the header fields that do not depend on ZStd, and the decompressed payloads
// Blob file = repeated { u32 nameLen, name, u64 dataLen, data } (same container as entropy_tool.cpp).  Pieces of a frame:
//   meta = int32 {w, h, nPlanes}; _mip_has_chunk (u8), _mip_tile_bbox (4 x int16), _mip_bitmap; alpha_mode (int32), alpha_bbox (4 x int32),
//   alpha_payload (all three or none); grad_bitmap_<i>, grad_rgbraw_<i> for i = 0..6; d1_pix, d1_type.
// The colour payloads come from grad_palette_<i> where the file has them; otherwise the host PaletteCompressor makes them from the raw colour
// streams, from a reset book and in pass order, as the device coder does for a frame of a batch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "encode_frame.h"
#include "palette.h"
#include "yaik_format.h"
#include "zstd_dl.h"

using namespace yaikfmt;
typedef std::vector<u8> Bytes;
typedef std::map<std::string, Bytes> Blobs;

static bool readAll(const char* path, Bytes& out) {
    FILE* f = fopen(path, "rb"); if (!f) return false;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    const bool ok = n == 0 || fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f); return ok;
}
static bool readBlobs(const char* path, Blobs& m) {
    Bytes all;
    if (!readAll(path, all)) return false;
    size_t p = 0;
    while (p + 4 <= all.size()) {
        u32 nl; memcpy(&nl, &all[p], 4); p += 4;
        if (p + nl + 8 > all.size()) return false;
        std::string name((const char*)&all[p], nl); p += nl;
        unsigned long long dl; memcpy(&dl, &all[p], 8); p += 8;
        if (p + dl > all.size()) return false;
        m[name] = Bytes(all.begin() + p, all.begin() + p + dl); p += dl;
    }
    return true;
}
static FILE* gOut;
static void blob(const std::string& name, const void* data, size_t len) {
    const u32 nl = (u32)name.size(); const unsigned long long dl = len;
    fwrite(&nl, 4, 1, gOut); fwrite(name.data(), 1, nl, gOut); fwrite(&dl, 8, 1, gOut); if (len) fwrite(data, 1, len, gOut);
}
static std::string key(const char* b, int i) { return std::string(b) + std::to_string(i); }

// the pointers of `p` point into `b` (and into `pal` for payloads made here)
static bool pieces(Blobs& b, Bytes pal[7], yaikenc::FramePieces& p) {
    if (b["meta"].size() != 12) { fprintf(stderr, "no meta blob\n"); return false; }
    int meta[3]; memcpy(meta, b["meta"].data(), 12);
    p.width = meta[0]; p.height = meta[1]; p.hasAlpha = meta[2] == 4;
    if (p.hasAlpha && b.count("_mip_has_chunk") && b["_mip_has_chunk"].size() == 1 && b["_mip_has_chunk"][0] && b["_mip_tile_bbox"].size() == 8) {
        s16 tb[4]; memcpy(tb, b["_mip_tile_bbox"].data(), 8);
        p.mipHasChunk = true;
        for (int k = 0; k < 4; k++) p.mipBox[k] = tb[k];
        p.mipBits = b["_mip_bitmap"].data(); p.mipBytes = b["_mip_bitmap"].size();
    }
    if (p.hasAlpha && b.count("alpha_mode") && b["alpha_mode"].size() == 4 && b["alpha_bbox"].size() == 16) {
        memcpy(&p.alphaMode, b["alpha_mode"].data(), 4);
        memcpy(p.alphaBox, b["alpha_bbox"].data(), 16);
        p.alpha = b["alpha_payload"].data(); p.alphaBytes = b["alpha_payload"].size();
    }
    PaletteResetCodeBook();
    for (int i = 0; i < 7; i++) {
        Bytes& bm = b[key("grad_bitmap_", i)]; Bytes& rgb = b[key("grad_rgbraw_", i)];
        p.bitmap[i] = bm.data(); p.bitmapBytes[i] = bm.size(); p.rgbBytes[i] = rgb.size();
        if (b.count(key("grad_palette_", i))) pal[i] = b[key("grad_palette_", i)];
        else if (!rgb.empty()) {
            pal[i].resize(rgb.size() * 3);
            u32 n = (u32)pal[i].size();
            Bytes copy = rgb;
            if (!PaletteCompressor(copy.data(), (int)copy.size(), pal[i].data(), &n)) { fprintf(stderr, "PaletteCompressor overflow\n"); return false; }
            pal[i].resize(n);
        }
        p.palette[i] = pal[i].data(); p.paletteBytes[i] = pal[i].size();
    }
    p.pix = b["d1_pix"].data(); p.pixBytes = b["d1_pix"].size(); p.type = b["d1_type"].data(); p.typeBytes = b["d1_type"].size();
    return true;
}

static int encode(int level, int threads, const char* prefix, int n, char** paths) {
    if (level < 0 || level > 22 || threads < 1 || threads > 16) { fprintf(stderr, "level 0..22 and threads 1..16\n"); return 2; }
    std::vector<Blobs> blobs((size_t)n);
    std::vector<std::vector<Bytes>> pal((size_t)n, std::vector<Bytes>(7));
    std::vector<yaikenc::FramePieces> fp((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!readBlobs(paths[i], blobs[(size_t)i])) { fprintf(stderr, "cannot read %s\n", paths[i]); return 2; }
        if (!pieces(blobs[(size_t)i], pal[(size_t)i].data(), fp[(size_t)i])) return 2;
    }
    std::vector<Bytes> out; int failed = -1; std::string err;
    if (!yaikenc::encodeFrames(fp.data(), n, level, threads, out, &failed, err)) { fprintf(stderr, "failed %d: %s\n", failed, err.c_str()); return 3; }
    for (int i = 0; i < n; i++) {
        const std::string name = std::string(prefix) + std::to_string(i) + ".yaik";
        FILE* f = fopen(name.c_str(), "wb"); if (!f) { fprintf(stderr, "cannot write %s\n", name.c_str()); return 2; }
        const bool ok = fwrite(out[(size_t)i].data(), 1, out[(size_t)i].size(), f) == out[(size_t)i].size();
        fclose(f);
        if (!ok) return 2;
    }
    return 0;
}

static bool expand(Bytes& dst, size_t n, const u8* z, size_t zn, const u8* end, int chunk, const char* what) {
    dst.resize(n);
    if (z + zn > end || !yaikzstd::decompress(dst.data(), n, z, zn)) { fprintf(stderr, "chunk %d: %s does not expand\n", chunk, what); return false; }
    return true;
}

static int parse(const char* path, const char* outPath) {
    Bytes f; if (!readAll(path, f)) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    if (f.size() < sizeof(FileHeader)) { fprintf(stderr, "no file header\n"); return 3; }
    FileHeader fh; memcpy(&fh, f.data(), sizeof fh);
    if (fh.tag != TAG_FILE) { fprintf(stderr, "no file header\n"); return 3; }
    gOut = fopen(outPath, "wb"); if (!gOut) return 2;
    const int w = fh.width, h = fh.height;
    { const int v[4] = { fh.version, fh.width, fh.height, fh.infoMask }; blob("file_header", v, sizeof v); }
    const u8* end = f.data() + f.size();
    size_t p = sizeof fh; int i = 0, terminated = 0;
    while (p + 4 <= f.size()) {
        u32 tag; memcpy(&tag, &f[p], 4);
        if (tag == TAG_END) { terminated = 1; p += 4; break; }
        if (p + sizeof(HeaderBase) > f.size()) break;
        HeaderBase hb; memcpy(&hb, &f[p], sizeof hb);
        const u8* body = &f[p] + sizeof hb;
        if (body + hb.length > end) { fprintf(stderr, "chunk %d: truncated\n", i); return 3; }
        const std::string c = "c" + std::to_string(i) + "_";
        blob(c + "tag", &hb.tag, 4);
        Bytes a, b2;
        size_t used = 0;                                                     // header + streams: the rest of the chunk is padding
        if (hb.tag == TAG_MIPMAP) {
            MipmapHeader mh; memcpy(&mh, body, sizeof mh);
            const int v[6] = { mh.bbox.x, mh.bbox.y, mh.bbox.w, mh.bbox.h, mh.version, mh.mipmapLevel };
            blob(c + "hdr", v, sizeof v);
            used = hb.length;                                                // the bit count is not in the header when the box is degenerate
            blob(c + "bits", body + sizeof mh, hb.length - sizeof mh);
        } else if (hb.tag == TAG_ALPHA) {
            AlphaHeader ah; memcpy(&ah, body, sizeof ah);
            const int v[8] = { ah.bbox.x, ah.bbox.y, ah.bbox.w, ah.bbox.h, (int)ah.expectedDecompressionSize, ah.version, ah.parameters, 0 };
            blob(c + "hdr", v, sizeof v);
            if (!expand(a, ah.expectedDecompressionSize, body + sizeof ah, ah.streamSize, end, i, "alpha")) return 3;
            blob(c + "alpha", a.data(), a.size());
            used = sizeof ah + ah.streamSize;
        } else if (hb.tag == TAG_GRADTILE) {
            HeaderGradientTile gh; memcpy(&gh, body, sizeof gh);
            const int v[10] = { gh.bbox.x, gh.bbox.y, gh.bbox.w, gh.bbox.h, (int)gh.streamRGBSizeCustomCompressor, (int)gh.streamRGBSizeUncompressed,
                                gh.colorCompression, gh.format, gh.plane, gh.version };
            blob(c + "hdr", v, sizeof v);
            u32 bx, by, bc;
            if (!swizzleSize(gh.format & 7, (gh.format >> 3) & 7, bx, by, bc)) { fprintf(stderr, "chunk %d: tile format\n", i); return 3; }
            const u8* z = body + sizeof gh;
            if (!expand(a, (size_t)((w + bx - 1) / bx) * ((h + by - 1) / by) * bc / 8, z, gh.streamBitmapSize, end, i, "bitmap")) return 3;
            if (!expand(b2, gh.streamRGBSizeCustomCompressor, z + gh.streamBitmapSize, gh.streamRGBSizeZStd, end, i, "palette")) return 3;
            blob(c + "bitmap", a.data(), a.size());
            blob(c + "palette", b2.data(), b2.size());
            used = sizeof gh + gh.streamBitmapSize + gh.streamRGBSizeZStd;
        } else if (hb.tag == TAG_TILE1D) {
            Header1D dh; memcpy(&dh, body, sizeof dh);
            const int v[5] = { (int)dh.streamPixelUncmp, (int)dh.streamTypeUncmp, dh.compressionColor, dh.compressionRange, dh.version };
            blob(c + "hdr", v, sizeof v);
            const u8* z = body + sizeof dh;
            if (!expand(a, dh.streamTypeUncmp, z, dh.streamTypeCnt, end, i, "type")) return 3;
            if (!expand(b2, dh.streamPixelUncmp, z + dh.streamTypeCnt, dh.streamPixelBit, end, i, "pix")) return 3;
            blob(c + "type", a.data(), a.size());
            blob(c + "pix", b2.data(), b2.size());
            used = sizeof dh + dh.streamTypeCnt + dh.streamPixelBit;
        } else { fprintf(stderr, "chunk %d: unknown tag %08x\n", i, hb.tag); return 3; }
        if (used > hb.length || hb.length - used > 3 || (hb.length & 3)) { fprintf(stderr, "chunk %d: length\n", i); return 3; }
        int pad[2] = { (int)(hb.length - used), 0 };
        for (size_t k = used; k < hb.length; k++) pad[1] |= body[k];         // padding bytes are zero
        blob(c + "pad", pad, sizeof pad);
        p += sizeof hb + hb.length; i++;
    }
    const int tail[3] = { i, terminated, (int)(f.size() - p) };                // chunks, terminator seen, bytes behind it
    blob("chunk_count_terminated_rest", tail, sizeof tail);
    fclose(gOut);
    return 0;
}

int main(int argc, char** argv) {
    if (!yaikzstd::available()) { fprintf(stderr, "%s\n", yaikzstd::lastError()); return 4; }
    if (argc >= 6 && !strcmp(argv[1], "encode")) return encode(atoi(argv[2]), atoi(argv[3]), argv[4], argc - 5, argv + 5);
    if (argc == 4 && !strcmp(argv[1], "parse")) return parse(argv[2], argv[3]);
    fprintf(stderr, "usage: encode_frame_tool encode <level> <threads> <out prefix> <pieces.blobs>... | encode_frame_tool parse <file.yaik> <out.blobs>\n");
    return 2;
}
