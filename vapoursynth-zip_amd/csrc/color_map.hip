// vszip.ColorMap on gfx950 (src/vapoursynth/color_map.zig:36-46): Gray8 to false-colour RGB24 through a 256-entry table a channel.
// One plane of bytes in, three out: 4 bytes of traffic a sample, every byte touched once; the work is the gather.
//
// Table. The three byte tables travel in the kernel argument as ONE table of 256 dwords, r | g << 8 | b << 16, so a sample costs one
// gather instead of three. Every workgroup copies it into LDS (a dword a lane) and gathers with ds_read_b32.
//
// 32 lanes that hit random entries share banks, neighbouring samples of an image hit the same entry, which is a broadcast; the difference
// does not show in the kernel's time (natural image and noise within 3 %), and a conflict-free layout, the table 32 times with every
// lane reading its own bank, which every workgroup has to fill with 32 KiB first, was slower at every band height.
//
// Mapping. A workgroup of 256 lanes takes a band of rows of a frame, as many as fill it once (row_units.hpp), and walks the band's
// groups of 16 samples in raster order. A lane loads its 16 samples with one non-temporal 16-byte load, gathers 16 dwords, separates
// the channels in registers (v_perm_b32, seven for four samples) and stores 16 bytes to each of the three planes, non-temporal,
// consecutive lanes writing consecutive 16 bytes.
//
// Paths. A frame whose four bases and four pitches are multiples of 16 takes the group path for the w / 16 whole groups of a row and
// finishes the row's last w % 16 samples one by one; any other frame goes sample by sample throughout, with the same bits. Neither
// path reads or writes outside [0, w) x h.
#include <algorithm>
#include <climits>

#include "row_units.hpp"

namespace {

constexpr int kThreads = kRowUnitThreads;
constexpr int kPx = 16;

struct ColorMapFrame {
    const uint8_t *src;
    uint8_t *r, *g, *b;
    int ss, rs, gs, bs, w, h;
    short vec, rows;  // bases and pitches are multiples of 16 bytes; rows a workgroup
    int block0;
};
struct ColorMapParams : PlaneTable<ColorMapFrame> {
    uint32_t lut[256];  // r | g << 8 | b << 16
};

#if defined(__HIPCC__)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kThreads) void color_map_kernel(const ColorMapParams prm) {
    static_assert(kThreads == 256);
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = prm.lut[threadIdx.x];
    __syncthreads();

    const int wg = blockIdx.x;
    const ColorMapFrame &f = prm.p[vszip_find_plane(prm, wg)];
    const int y0 = (wg - f.block0) * f.rows, rows = min((int)f.rows, f.h - y0), w = f.w;
    const uint8_t *s = f.src + (size_t)y0 * f.ss;
    uint8_t *r = f.r + (size_t)y0 * f.rs, *g = f.g + (size_t)y0 * f.gs, *b = f.b + (size_t)y0 * f.bs;
    const int ss = f.ss, rs = f.rs, gs = f.gs, bs = f.bs;
    int x0 = 0;
    if (f.vec) {
        const int nv = w / kPx;
        for_each_row_unit(rows, nv, [&](int row, int i) {
            const size_t x = (size_t)i * kPx;
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s + (size_t)row * ss + x));
            u32x4 vr, vg, vb;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t q = v[k];
                const uint32_t t0 = tab[q & 255u], t1 = tab[(q >> 8) & 255u], t2 = tab[(q >> 16) & 255u], t3 = tab[q >> 24];
                const uint32_t rg01 = byte_perm(t1, t0, 0x05010400u), rg23 = byte_perm(t3, t2, 0x05010400u);  // r0 r1 g0 g1; r2 r3 g2 g3
                const uint32_t b01 = byte_perm(t1, t0, 0x0c0c0602u), b23 = byte_perm(t3, t2, 0x0c0c0602u);    // b0 b1 0 0; b2 b3 0 0
                vr[k] = byte_perm(rg23, rg01, 0x05040100u);
                vg[k] = byte_perm(rg23, rg01, 0x07060302u);
                vb[k] = byte_perm(b23, b01, 0x05040100u);
            }
            __builtin_nontemporal_store(vr, reinterpret_cast<u32x4 *>(r + (size_t)row * rs + x));
            __builtin_nontemporal_store(vg, reinterpret_cast<u32x4 *>(g + (size_t)row * gs + x));
            __builtin_nontemporal_store(vb, reinterpret_cast<u32x4 *>(b + (size_t)row * bs + x));
        });
        x0 = nv * kPx;
    }
    for_each_row_unit(rows, w - x0, [&](int row, int i) {
        const size_t x = (size_t)x0 + i;
        const uint32_t t = tab[s[(size_t)row * ss + x]];
        r[(size_t)row * rs + x] = (uint8_t)t;
        g[(size_t)row * gs + x] = (uint8_t)(t >> 8);
        b[(size_t)row * bs + x] = (uint8_t)(t >> 16);
    });
}
#endif  // __HIPCC__

}  // namespace

VSZIP_EXPORT int vszip_color_map(vszip_ctx *ctx, const vszip_color_map_frame *frames, int nframes, const uint8_t lut[3][256]) {
    if (!ctx || !frames || nframes <= 0) return VSZIP_ERR_ARG;
    if (!lut) return vszip_set_error(ctx, VSZIP_ERR_ARG, "ColorMap: lut must not be NULL");
    long long blocks = 0;
    for (int i = 0; i < nframes; ++i) {
        const vszip_color_map_frame &s = frames[i];
        if (!s.src || !s.r || !s.g || !s.b) return vszip_set_error(ctx, VSZIP_ERR_ARG, "ColorMap: frame %d: src, r, g and b must not be NULL", i);
        const ptrdiff_t lo = std::min(std::min(s.src_stride, s.r_stride), std::min(s.g_stride, s.b_stride)), hi = std::max(std::max(s.src_stride, s.r_stride), std::max(s.g_stride, s.b_stride));
        if (s.w < 1 || s.h < 1 || lo < s.w || hi > INT_MAX)
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "ColorMap: frame %d: bad geometry %dx%d, pitches %lld -> %lld / %lld / %lld", i, (int)s.w, (int)s.h, (long long)s.src_stride,
                                   (long long)s.r_stride, (long long)s.g_stride, (long long)s.b_stride);
        blocks += s.h;
    }
    if (blocks > INT_MAX / 2) return vszip_set_error(ctx, VSZIP_ERR_UNSUPPORTED, "ColorMap: %lld rows are more than one call numbers", blocks);
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ColorMapParams prm;  // the table is copied into the kernel argument: the caller's array is free when the call returns
    for (int i = 0; i < 256; ++i) prm.lut[i] = (uint32_t)lut[0][i] | ((uint32_t)lut[1][i] << 8) | ((uint32_t)lut[2][i] << 16);
    return vszip_for_each_table(
        ctx, prm, nframes,
        [&](ColorMapFrame &d, int i) -> int {
            const vszip_color_map_frame &s = frames[i];
            d.src = s.src;
            d.r = s.r;
            d.g = s.g;
            d.b = s.b;
            d.ss = (int)s.src_stride;
            d.rs = (int)s.r_stride;
            d.gs = (int)s.g_stride;
            d.bs = (int)s.b_stride;
            d.w = s.w;
            d.h = s.h;
            const uintptr_t bits = reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.r) | reinterpret_cast<uintptr_t>(s.g) | reinterpret_cast<uintptr_t>(s.b) |
                                   (uintptr_t)(s.src_stride | s.r_stride | s.g_stride | s.b_stride);
            d.vec = (bits & 15) == 0;
            d.rows = (short)vszip_rows_per_workgroup(d.vec ? s.w / kPx : s.w);
            return (s.h + d.rows - 1) / d.rows;
        },
        [&](const ColorMapParams &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            hipLaunchKernelGGL(color_map_kernel, dim3(blocks), dim3(kThreads), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}
