// Alpha values through the C++ drop-in, for tests:
//   alpha_driver enc <in.bin> <out.yaik> <emitAlpha 0|1> [parallel] [alpha6]
//        ConvertHotPath (or ConvertHotPathParallel with 4 threads) with the 'ALPM' opt-in off / on; alpha6 also sets alpha6Bit
//   alpha_driver dec <in.yaik> <out.bin>                                YAIK_DecodeImage, default builder then a custom builder; out.bin =
//        int32 {ok, errorCode, width, height, hasAlpha, bytesPerPixel, customOk, customErrorCode, customHasPlaneA, customStrideA}, the default
//        builder's image (w * h * bytesPerPixel), then the custom builder's planeA (w * h bytes) when it had one
//   in.bin: int32 w, h, nPlanes, then nPlanes planes of w * h int32
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "EncoderContext.h"
#include "yaik_decode.h"

static std::vector<uint8_t> gPlaneA;
static int gStrideA = 0, gHadA = 0;

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: alpha_driver enc|dec ...\n"); return 2; }
    const std::string cmd = argv[1];
    if (cmd == "enc" && argc >= 5) {
        FILE* fi = fopen(argv[2], "rb"); if (!fi) return 2;
        int hdr[3]; if (fread(hdr, 4, 3, fi) != 3) return 2;
        const int w = hdr[0], h = hdr[1], np = hdr[2];
        Image* img = Image::CreateImage(w, h, np, false);
        for (int p = 0; p < np; p++) if (fread(img->GetPlane(p)->GetPixels(), 4, (size_t)w * h, fi) != (size_t)w * h) return 2;
        fclose(fi);
        EncoderContext* ctx = new EncoderContext();
        if (!ctx->SetImageToEncode(img)) { fprintf(stderr, "%s\n", ctx->LastError()); return 3; }
        ctx->emitAlpha = atoi(argv[4]) != 0;
        FILE* f = fopen(argv[3], "wb"); if (!f) return 2;
        bool parallel = false;
        for (int i = 5; i < argc; i++) {
            const std::string opt = argv[i];
            if (opt == "parallel") parallel = true;
            else if (opt == "alpha6") ctx->alpha6Bit = true;
            else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        }
        const bool ok = parallel ? ctx->ConvertHotPathParallel(f, 4) : ctx->ConvertHotPath(f);
        fclose(f);
        if (!ok) { fprintf(stderr, "ConvertHotPath: %s\n", ctx->LastError()); return 4; }
        delete ctx;
        return 0;
    }
    if (cmd == "dec") {
        FILE* fi = fopen(argv[2], "rb"); if (!fi) return 2;
        fseek(fi, 0, SEEK_END); const long n = ftell(fi); fseek(fi, 0, SEEK_SET);
        std::vector<uint32_t> stream(((size_t)n + 3) / 4 + 1);
        if (fread(stream.data(), 1, (size_t)n, fi) != (size_t)n) return 2;
        fclose(fi);
        YAIK_LIB lib = YAIK_Init(1, nullptr);
        if (!lib) return 5;
        int32_t res[10] = {};
        std::vector<uint8_t> img;
        YAIK_SDecodedImage di;
        if (YAIK_DecodeImagePre(lib, stream.data(), (uint32_t)n, &di)) {
            res[2] = di.width; res[3] = di.height; res[4] = di.hasAlpha ? 1 : 0;
            img.assign((size_t)di.width * di.height * 4, 0);
            di.outputImage = img.data(); di.outputImageStride = di.width * 4;
            res[0] = YAIK_DecodeImage(stream.data(), (uint32_t)n, &di) ? 1 : 0;
        }
        res[1] = (int)YAIK_GetErrorCode();
        if (YAIK_DecodeImagePre(lib, stream.data(), (uint32_t)n, &di)) {
            std::vector<uint8_t> dummy((size_t)di.width * di.height * 4);
            di.outputImage = dummy.data(); di.outputImageStride = di.width * 4;
            di.customImageOutput = [](YAIK_SDecodedImage* u, YAIK_SCustomDataSource* s) {
                gHadA = s->planeA != nullptr; gStrideA = s->strideA;
                if (s->planeA) gPlaneA.assign(s->planeA, s->planeA + (size_t)u->width * u->height);
            };
            res[6] = YAIK_DecodeImage(stream.data(), (uint32_t)n, &di) ? 1 : 0;
        }
        res[7] = (int)YAIK_GetErrorCode(); res[8] = gHadA; res[9] = gStrideA;
        // the default builder writes RGB (3 B/pixel) rows without an 'ALPM' chunk and RGBA with one; the stride was 4 B/pixel either way
        const int bpp = res[0] && !gPlaneA.empty() ? 4 : 3;
        res[5] = bpp;
        FILE* fo = fopen(argv[3], "wb"); if (!fo) return 2;
        fwrite(res, 4, 10, fo);
        if (res[0])
            for (int y = 0; y < res[3]; y++) fwrite(img.data() + (size_t)y * res[2] * 4, 1, (size_t)res[2] * bpp, fo);
        if (gHadA) fwrite(gPlaneA.data(), 1, gPlaneA.size(), fo);
        fclose(fo);
        YAIK_Release(lib);
        return 0;
    }
    return 2;
}
