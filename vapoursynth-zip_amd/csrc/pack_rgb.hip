// vszip.PackRGB on gfx950 (src/vapoursynth/packrgb.zig:33-63): planar RGB24 or RGB30 to one packed 32-bit plane. Three planes of 8- or
// 16-bit samples in, one plane of four bytes a sample out: 7 or 10 bytes of traffic a sample, every byte touched once.
//
// Mapping. A lane owns a group of four samples: one dword (8-bit) or two (16-bit) from each plane, loaded with the non-temporal hint,
// interleaved in registers (8-bit: v_perm_b32, six for four samples, the 0xFF of the fourth byte coming out of the selector; 10-bit:
// shifts and ors in 32-bit arithmetic, nothing masked, as the reference writes it) and stored as ONE 16-byte non-temporal store, so
// consecutive lanes write consecutive 16 bytes and a wave's store is 1 KiB of a row. A workgroup of 256 lanes takes a band of rows of a
// frame and walks the band's groups in raster order (row_units.hpp); the band is as many rows as fill the workgroup once (one row from
// 1024 samples on), which measured fastest (16 samples a lane, whose four stores a lane lie 64 bytes apart, reached
// 0.37-0.56 of this mapping's rate).
//
// Paths. A frame whose four bases and four pitches (in bytes) are multiples of 16 takes the group path for the w / 4 whole groups of
// a row and finishes the row's last w % 4 samples one by one; any other frame goes sample by sample throughout, with the same bits.
// Neither path reads or writes outside [0, w) x h. r, g and b may be the same plane.
#include <algorithm>
#include <climits>
#include <type_traits>

#include "row_units.hpp"

namespace {

constexpr int kThreads = kRowUnitThreads;
constexpr int kPx = 4;  // samples a lane and access

struct PackFrame {
    const void *r, *g, *b;
    uint32_t *dst;
    int rs, gs, bs, ds, w, h;  // pitches in samples of the plane's own type
    short vec, rows;           // bases and pitches are multiples of 16 bytes; rows a workgroup
    int block0;
};
using PackParams = PlaneTable<PackFrame>;

#if defined(__HIPCC__)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t pack1(uint8_t r, uint8_t g, uint8_t b) { return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16) | (255u << 24); }
__device__ __forceinline__ uint32_t pack1(uint16_t r, uint16_t g, uint16_t b) { return (uint32_t)b | ((uint32_t)g << 10) | ((uint32_t)r << 20) | (3u << 30); }

// four 8-bit samples of each plane, a dword each -> four packed samples
__device__ __forceinline__ u32x4 pack4(uint32_t r, uint32_t g, uint32_t b) {
    const uint32_t bg01 = byte_perm(g, b, 0x05010400u), bg23 = byte_perm(g, b, 0x07030602u);  // b0 g0 b1 g1; b2 g2 b3 g3
    u32x4 o;
    o.x = byte_perm(r, bg01, 0x0d040100u);
    o.y = byte_perm(r, bg01, 0x0d050302u);
    o.z = byte_perm(r, bg23, 0x0d060100u);
    o.w = byte_perm(r, bg23, 0x0d070302u);
    return o;
}
// four 16-bit samples of each plane, two dwords each
__device__ __forceinline__ u32x4 pack4(u32x2 r, u32x2 g, u32x2 b) {
    u32x4 o;
    o.x = pack1((uint16_t)r.x, (uint16_t)g.x, (uint16_t)b.x);
    o.y = pack1((uint16_t)(r.x >> 16), (uint16_t)(g.x >> 16), (uint16_t)(b.x >> 16));
    o.z = pack1((uint16_t)r.y, (uint16_t)g.y, (uint16_t)b.y);
    o.w = pack1((uint16_t)(r.y >> 16), (uint16_t)(g.y >> 16), (uint16_t)(b.y >> 16));
    return o;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void pack_rgb_kernel(const PackParams prm) {
    using Quad = std::conditional_t<sizeof(T) == 1, uint32_t, u32x2>;  // four samples of a plane
    const int wg = blockIdx.x;
    const PackFrame &f = prm.p[vszip_find_plane(prm, wg)];
    const int y0 = (wg - f.block0) * f.rows, rows = min((int)f.rows, f.h - y0), w = f.w;
    const T *r = static_cast<const T *>(f.r) + (size_t)y0 * f.rs, *g = static_cast<const T *>(f.g) + (size_t)y0 * f.gs, *b = static_cast<const T *>(f.b) + (size_t)y0 * f.bs;
    uint32_t *d = f.dst + (size_t)y0 * f.ds;
    const int rs = f.rs, gs = f.gs, bs = f.bs, ds = f.ds;
    int x0 = 0;
    if (f.vec) {
        const int nv = w / kPx;
        for_each_row_unit(rows, nv, [&](int row, int i) {
            const size_t x = (size_t)i * kPx;
            const Quad vr = __builtin_nontemporal_load(reinterpret_cast<const Quad *>(r + (size_t)row * rs + x)),
                       vg = __builtin_nontemporal_load(reinterpret_cast<const Quad *>(g + (size_t)row * gs + x)),
                       vb = __builtin_nontemporal_load(reinterpret_cast<const Quad *>(b + (size_t)row * bs + x));
            __builtin_nontemporal_store(pack4(vr, vg, vb), reinterpret_cast<u32x4 *>(d + (size_t)row * ds + x));
        });
        x0 = nv * kPx;
    }
    for_each_row_unit(rows, w - x0, [&](int row, int i) {
        const size_t x = (size_t)x0 + i;
        d[(size_t)row * ds + x] = pack1(r[(size_t)row * rs + x], g[(size_t)row * gs + x], b[(size_t)row * bs + x]);
    });
}
#endif  // __HIPCC__

template <typename T>
int pack_rgb_run(vszip_ctx *ctx, const vszip_pack_rgb_frame *frames, int nframes) {
    PackParams prm;
    return vszip_for_each_table(
        ctx, prm, nframes,
        [&](PackFrame &d, int i) -> int {
            const vszip_pack_rgb_frame &s = frames[i];
            d.r = s.r;
            d.g = s.g;
            d.b = s.b;
            d.dst = s.dst;
            d.rs = (int)s.r_stride;
            d.gs = (int)s.g_stride;
            d.bs = (int)s.b_stride;
            d.ds = (int)s.dst_stride;
            d.w = s.w;
            d.h = s.h;
            const uintptr_t bits = reinterpret_cast<uintptr_t>(s.r) | reinterpret_cast<uintptr_t>(s.g) | reinterpret_cast<uintptr_t>(s.b) | reinterpret_cast<uintptr_t>(s.dst) |
                                   (uintptr_t)((s.r_stride | s.g_stride | s.b_stride) * (ptrdiff_t)sizeof(T)) | (uintptr_t)(s.dst_stride * 4);
            d.vec = (bits & 15) == 0;
            d.rows = (short)vszip_rows_per_workgroup(d.vec ? s.w / kPx : s.w);
            return (s.h + d.rows - 1) / d.rows;
        },
        [&](const PackParams &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            hipLaunchKernelGGL(pack_rgb_kernel<T>, dim3(blocks), dim3(kThreads), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}

}  // namespace

VSZIP_EXPORT int vszip_pack_rgb(vszip_ctx *ctx, int bits, const vszip_pack_rgb_frame *frames, int nframes) {
    if (!ctx || !frames || nframes <= 0) return VSZIP_ERR_ARG;
    if (bits != 8 && bits != 10) return vszip_set_error(ctx, VSZIP_ERR_ARG, "PackRGB: only RGB24 and RGB30 inputs are supported!");
    long long rows = 0;
    for (int i = 0; i < nframes; ++i) {
        const vszip_pack_rgb_frame &s = frames[i];
        if (!s.r || !s.g || !s.b || !s.dst) return vszip_set_error(ctx, VSZIP_ERR_ARG, "PackRGB: frame %d: r, g, b and dst must not be NULL", i);
        const ptrdiff_t lo = std::min(std::min(s.r_stride, s.g_stride), std::min(s.b_stride, s.dst_stride)), hi = std::max(std::max(s.r_stride, s.g_stride), std::max(s.b_stride, s.dst_stride));
        if (s.w < 1 || s.h < 1 || lo < s.w || hi > INT_MAX)
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "PackRGB: frame %d: bad geometry %dx%d, pitches %lld / %lld / %lld -> %lld", i, (int)s.w, (int)s.h, (long long)s.r_stride,
                                   (long long)s.g_stride, (long long)s.b_stride, (long long)s.dst_stride);
        rows += s.h;
    }
    if (rows > INT_MAX / 2) return vszip_set_error(ctx, VSZIP_ERR_UNSUPPORTED, "PackRGB: %lld rows are more than one call numbers", rows);
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return bits == 8 ? pack_rgb_run<uint8_t>(ctx, frames, nframes) : pack_rgb_run<uint16_t>(ctx, frames, nframes);
}
