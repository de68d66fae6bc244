// Stand-alone host check of the Compress block body (vapoursynth-zip_amd/csrc/compress_block.hpp, the very text the kernel runs per
// lane) and of vszip_compress_tables (host_params.cpp), built under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_compress_block_host.py.
//   compress_block_check IN OUT codec qscale dc_prec quality chroma
// IN holds N x 64 bytes, the samples of N blocks in raster order; OUT receives the N x 64 samples of the round trip, which the
// Python side compares with the numpy spec's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/vszip_hip.h"
#include "../vapoursynth-zip_amd/csrc/compress_block.hpp"

template <int CODEC>
static void run(const std::vector<uint8_t> &in, std::vector<uint8_t> &out, const struct vszip_compress_tables &tb, int idx) {
    for (size_t n = 0; n + 64 <= in.size(); n += 64) {
        int32_t b[64];
        uint8_t o[64];
        for (int i = 0; i < 64; ++i) b[i] = (int32_t)in[n + i] - (CODEC == 1 ? 128 : 0);
        vszip_compress_dsp::process_block<CODEC>(b, o, tb.qmul[idx], tb.deq[idx], tb.dc_q, tb.dc_scale);
        for (int i = 0; i < 64; ++i) out[n + i] = o[i];
    }
}

int main(int argc, char **argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: compress_block_check IN OUT codec qscale dc_prec quality chroma\n");
        return 2;
    }
    struct vszip_compress_tables tb;
    char err[128] = "";
    if (vszip_compress_tables(std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), &tb, err, sizeof err) != VSZIP_OK) {
        std::fprintf(stderr, "%s\n", err);
        return 3;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 4;
    std::vector<uint8_t> in;
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + n);
    std::fclose(f);
    if (in.empty() || in.size() % 64) return 5;
    std::vector<uint8_t> out(in.size());
    const int idx = std::atoi(argv[7]) != 0;
    if (tb.codec == 0)
        run<0>(in, out, tb, idx);
    else
        run<1>(in, out, tb, idx);
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 6;
    std::fclose(f);
    std::printf("%zu blocks\n", out.size() / 64);
    return 0;
}
