// vszip.Compress on gfx950 (src/filters/compress.zig as called by src/vapoursynth/compress.zig): every 8 x 8 block of an 8-bit
// plane through forward DCT, quantiser, dequantiser and inverse DCT of MPEG-2 intra or JPEG. One fused pass: a block is loaded,
// transformed and stored, no intermediate plane exists.
//
// Mapping. A LANE owns a block: its 64 values stay in the lane's registers through all four 1-D passes, so the transposes between
// the passes are register renaming, there is no LDS, no cross-lane move and no barrier. Blocks are numbered in raster order over
// the plane and a workgroup of 256 lanes takes 256 consecutive blocks, so a wave's load of one block row covers 512 consecutive
// bytes of a plane row (8 bytes a lane), the last wave of a block row running on into the next. Every index into the block is a
// compile-time constant after unrolling; the quantiser tables travel in the kernel argument beside the plane table and are read
// with scalar loads at constant offsets (luma or chroma is a property of the plane, so of the whole workgroup).
//
// Paths. A full block of a plane whose src and dst bases and pitches are multiples of 8 is loaded and stored as eight 64-bit
// words. Any other block goes byte by byte: a partial block at the right or bottom edge reads min(x, w - 1) / min(y, h - 1) and
// stores only what lies inside the plane, and a plane of any other alignment takes this path for every block, with the same
// bits. Neither path reads or writes outside [0, w) x h. dst == src is served: a lane has read all of its block before it stores,
// and no other lane touches that block.
#include <algorithm>
#include <climits>
#include <cstring>

#include "compress_block.hpp"
#include "plane_table.hpp"

namespace {

constexpr int kThreads = 256;

struct CompressPlane {
    const uint8_t *src;
    uint8_t *dst;
    int sstride, dstride, w, h;
    int nbx, nblocks;  // blocks per block row; blocks of the plane
    short chroma, vec;  // table index; bases and pitches are multiples of 8
    int block0;
};
struct CompressParams : PlaneTable<CompressPlane> {
    int32_t qmul[2][64], deq[2][64];
    int32_t dc_q, dc_scale;
};

#if defined(__HIPCC__)
template <int CODEC>
__global__ __launch_bounds__(kThreads) void compress_kernel(const CompressParams prm) {
    using namespace vszip_compress_dsp;
    const int wg = blockIdx.x;
    const CompressPlane &pl = prm.p[vszip_find_plane(prm, wg)];
    const int g = (wg - pl.block0) * kThreads + (int)threadIdx.x;
    if (g >= pl.nblocks) return;
    const int by = g / pl.nbx, bx = g - by * pl.nbx;
    const int x0 = bx * 8, y0 = by * 8, w = pl.w, h = pl.h;
    const bool fast = pl.vec && x0 + 8 <= w && y0 + 8 <= h;
    constexpr i32 kLevel = CODEC == 1 ? 128 : 0;
    i32 b[64];
    if (fast) {
        const uint8_t *s = pl.src + (size_t)y0 * pl.sstride + x0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint2 v = *reinterpret_cast<const uint2 *>(s + (size_t)r * pl.sstride);
#pragma unroll
            for (int k = 0; k < 8; ++k) b[8 * r + k] = (i32)(((k < 4 ? v.x : v.y) >> (8 * (k & 3))) & 255u) - kLevel;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint8_t *s = pl.src + (size_t)std::min(y0 + r, h - 1) * pl.sstride;
#pragma unroll
            for (int k = 0; k < 8; ++k) b[8 * r + k] = (i32)s[std::min(x0 + k, w - 1)] - kLevel;
        }
    }
    uint8_t out[64];
    process_block<CODEC>(b, out, prm.qmul[pl.chroma], prm.deq[pl.chroma], prm.dc_q, prm.dc_scale);
    if (fast) {
        uint8_t *d = pl.dst + (size_t)y0 * pl.dstride + x0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint2 v;
            v.x = (uint32_t)out[8 * r] | ((uint32_t)out[8 * r + 1] << 8) | ((uint32_t)out[8 * r + 2] << 16) | ((uint32_t)out[8 * r + 3] << 24);
            v.y = (uint32_t)out[8 * r + 4] | ((uint32_t)out[8 * r + 5] << 8) | ((uint32_t)out[8 * r + 6] << 16) | ((uint32_t)out[8 * r + 7] << 24);
            *reinterpret_cast<uint2 *>(d + (size_t)r * pl.dstride) = v;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint8_t *d = pl.dst + (size_t)(y0 + r) * pl.dstride;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (y0 + r < h && x0 + k < w) d[x0 + k] = out[8 * r + k];
        }
    }
}
#endif  // __HIPCC__

}  // namespace

VSZIP_EXPORT int vszip_compress(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, const struct vszip_compress_tables *tables, const uint8_t *chroma) {
    if (!ctx || !planes || nplanes <= 0) return VSZIP_ERR_ARG;
    if (!tables) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Compress: tables must not be NULL");
    if (tables->codec < 0 || tables->codec > 1) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Compress: codec must be 0 (mpeg2) or 1 (jpeg).");
    if (tables->codec == 0 && tables->dc_q <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Compress: dc_q must be positive");
    for (int p = 0; p < 2; ++p)
        for (int i = 0; i < 64; ++i)
            if (tables->qmul[p][i] < 0 || tables->qmul[p][i] > vszip_compress_dsp::kMaxQmul || tables->deq[p][i] < 0 || tables->deq[p][i] > vszip_compress_dsp::kMaxDeq)
                return vszip_set_error(ctx, VSZIP_ERR_ARG, "Compress: tables: qmul[%d][%d] = %d, deq = %d are outside 0..%d, 0..%d", p, i, (int)tables->qmul[p][i],
                                       (int)tables->deq[p][i], vszip_compress_dsp::kMaxQmul, vszip_compress_dsp::kMaxDeq);
    for (int i = 0; i < nplanes; ++i) {
        const vszip_plane &s = planes[i];
        if (!s.src || !s.dst) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Compress: plane %d: src and dst must not be NULL", i);
        if (s.w < 1 || s.h < 1 || s.src_stride < s.w || s.dst_stride < s.w || s.src_stride > INT_MAX || s.dst_stride > INT_MAX)
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "Compress: plane %d: bad geometry %dx%d, pitches %lld / %lld", i, (int)s.w, (int)s.h, (long long)s.src_stride,
                                   (long long)s.dst_stride);
        if ((long long)((s.w + 7LL) / 8) * ((s.h + 7LL) / 8) > INT_MAX / 2)
            return vszip_set_error(ctx, VSZIP_ERR_UNSUPPORTED, "Compress: plane %d: %dx%d has more blocks than one launch numbers", i, (int)s.w, (int)s.h);
    }
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    CompressParams prm;  // the tables are copied into the kernel argument: the caller's struct is free when the call returns
    memcpy(prm.qmul, tables->qmul, sizeof prm.qmul);
    memcpy(prm.deq, tables->deq, sizeof prm.deq);
    prm.dc_q = tables->dc_q;
    prm.dc_scale = tables->dc_scale;
    const int codec = tables->codec;
    return vszip_for_each_table(
        ctx, prm, nplanes,
        [&](CompressPlane &d, int i) -> int {
            const vszip_plane &s = planes[i];
            d.src = static_cast<const uint8_t *>(s.src);
            d.dst = static_cast<uint8_t *>(s.dst);
            d.sstride = (int)s.src_stride;
            d.dstride = (int)s.dst_stride;
            d.w = s.w;
            d.h = s.h;
            d.nbx = (s.w + 7) / 8;
            d.nblocks = d.nbx * ((s.h + 7) / 8);
            d.chroma = chroma ? (short)(chroma[i] != 0) : 0;
            d.vec = ((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst) | (uintptr_t)s.src_stride | (uintptr_t)s.dst_stride) & 7) == 0;
            return (d.nblocks + kThreads - 1) / kThreads;
        },
        [&](const CompressParams &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            if (codec == 0)
                hipLaunchKernelGGL(compress_kernel<0>, dim3(blocks), dim3(kThreads), 0, ctx->stream, t);
            else
                hipLaunchKernelGGL(compress_kernel<1>, dim3(blocks), dim3(kThreads), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}
