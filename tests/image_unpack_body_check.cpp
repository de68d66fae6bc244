// Stand-alone host check of the ImageUnpack lane bodies (vapoursynth-zip_amd/csrc/image_unpack_body.hpp, the very text every lane of
// the kernels runs), built under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_image_unpack_body_host.py.
//   image_unpack_body_check IN OUT PAL S C w h src_pitch vec src_bits
// IN holds the packed source: (h - 1) x src_pitch + w x C x S bytes, and lives in a heap block of exactly that size, as every output
// plane lives in one of exactly (h - 1) x pitch + w samples (vec 1: pitch = w rounded up to 16 bytes, the unit path; vec 0: pitch = w,
// pixel by pixel), so a read or write one byte too far is a sanitizer report. PAL: 1024 bytes (256 x R, G, B, A) for the INDEXED body
// (then S = C = 1), or "-". The bodies run for tid = 0 .. 255 of every band (vszip_rows_per_workgroup rows, as the library cuts them), every lane of a workgroup before the next
// step where the kernel has a barrier, with the LDS of the several-channel kernels as a heap block of the kernel's size. OUT receives the planes, dense, one after
// another in the pixel's memory order (INDEXED: R, G, B, A), which the Python side compares with the numpy spec's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vapoursynth-zip_amd/csrc/image_unpack_body.hpp"

namespace iu = image_unpack;

template <int S>
static void run_grey(const iu::UnpackFrame &f, int bands, uint32_t mask4, uint32_t mul) {
    for (int b = 0; b < bands; ++b)
        for (int tid = 0; tid < iu::kThreads; ++tid) iu::grey_lane<S>(f, b, tid, mask4, mul);
}

// several channels: what the kernel does around its barriers, with the LDS as a heap block of the kernel's size
template <int S, int C>
static void run_staged(const iu::UnpackFrame &f, int bands) {
    const size_t lds_bytes = (size_t)iu::staged_chunks(C) * 16;
    void *lds = nullptr;
    if (posix_memalign(&lds, 16, lds_bytes) != 0) std::exit(5);
    for (int b = 0; b < bands; ++b) {
        const iu::Band<S, C> band(f, b);
        const int sweeps = iu::staged_sweeps(band);
        for (int t = 0; t < sweeps; ++t) {
            std::memset(lds, 0xEE, lds_bytes);
            for (int tid = 0; tid < iu::kThreads; ++tid) iu::stage_sweep(band, t, tid, static_cast<uint32_t *>(lds));
            for (int tid = 0; tid < iu::kThreads; ++tid) iu::unpack_sweep(band, t, tid, static_cast<const uint32_t *>(lds));
        }
        for (int tid = 0; tid < iu::kThreads; ++tid) iu::staged_tail(band, tid);
    }
    std::free(lds);
}

int main(int argc, char **argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: image_unpack_body_check IN OUT PAL S C w h src_pitch vec src_bits\n");
        return 2;
    }
    const int S = std::atoi(argv[4]), C = std::atoi(argv[5]), w = std::atoi(argv[6]), h = std::atoi(argv[7]), spitch = std::atoi(argv[8]), vec = std::atoi(argv[9]),
              bits = std::atoi(argv[10]), rows = vszip_rows_per_workgroup(vec ? w / (16 / (S > 0 ? S : 1)) : w);
    const bool indexed = std::strcmp(argv[3], "-") != 0;
    if (w < 1 || h < 1 || spitch < w * C * S || (S != 1 && S != 2 && S != 4) || C < 1 || C > 4) return 2;
    const size_t in_bytes = (size_t)(h - 1) * spitch + (size_t)w * C * S;
    uint8_t *in = static_cast<uint8_t *>(std::malloc(in_bytes));
    FILE *fp = std::fopen(argv[1], "rb");
    if (!in || !fp || std::fread(in, 1, in_bytes, fp) != in_bytes || std::fgetc(fp) != EOF) return 4;
    std::fclose(fp);
    std::vector<uint32_t> tab;
    if (indexed) {
        uint8_t pal[1024];
        fp = std::fopen(argv[3], "rb");
        if (!fp || std::fread(pal, 1, sizeof pal, fp) != sizeof pal) return 4;
        std::fclose(fp);
        for (int i = 0; i < 256; ++i) tab.push_back((uint32_t)pal[4 * i] | ((uint32_t)pal[4 * i + 1] << 8) | ((uint32_t)pal[4 * i + 2] << 16) | ((uint32_t)pal[4 * i + 3] << 24));
    }
    const int nout = indexed ? 4 : C, opitch = vec ? (w * S + 15) / 16 * 16 / S : w;
    const size_t out_bytes = ((size_t)(h - 1) * opitch + w) * S;
    iu::UnpackFrame f = {};
    f.src = in;
    f.ss = spitch;
    for (int c = 0; c < nout; ++c) {
        void *p = nullptr;
        if (posix_memalign(&p, 16, out_bytes) != 0) return 5;
        std::memset(p, 0xEE, out_bytes);
        f.o[c] = p;
        f.os[c] = opitch;
    }
    f.w = w;
    f.h = h;
    f.vec = (short)vec;
    f.rows = (short)rows;
    const int bands = (h + rows - 1) / rows;
    const uint32_t m = (1u << (bits < 8 ? bits : 8)) - 1u, mask4 = m * 0x01010101u, mul = 255u / m;
    if (indexed) {
        for (int b = 0; b < bands; ++b)
            for (int tid = 0; tid < iu::kThreads; ++tid) iu::band_lane_indexed(f, b, tid, tab.data());
    } else {
        switch (S * 10 + C) {
            case 11: run_grey<1>(f, bands, mask4, mul); break;
            case 21: run_grey<2>(f, bands, mask4, mul); break;
            case 12: run_staged<1, 2>(f, bands); break;
            case 13: run_staged<1, 3>(f, bands); break;
            case 14: run_staged<1, 4>(f, bands); break;
            case 22: run_staged<2, 2>(f, bands); break;
            case 23: run_staged<2, 3>(f, bands); break;
            case 24: run_staged<2, 4>(f, bands); break;
            case 44: run_staged<4, 4>(f, bands); break;
            default: return 2;
        }
    }
    fp = std::fopen(argv[2], "wb");
    if (!fp) return 6;
    for (int c = 0; c < nout; ++c) {
        for (int y = 0; y < h; ++y)
            if (std::fwrite(static_cast<uint8_t *>(f.o[c]) + (size_t)y * opitch * S, 1, (size_t)w * S, fp) != (size_t)w * S) return 6;
        std::free(f.o[c]);
    }
    std::fclose(fp);
    std::free(in);
    std::printf("%d planes of %dx%d\n", nout, w, h);
    return 0;
}
