// vszip.ImageRead's pixel loop on gfx950 (src/vapoursynth/image_read.zig:38-91, dispatched at :285-345): a decoder's packed, interleaved
// pixels to planes plus an alpha plane. One packed buffer in, up to four planes out, every byte touched once; the mirror of pack_rgb.hip.
//
// Mapping. A pixel is C samples of S bytes. A lane owns a unit of 16 / S pixels (16 of 8 bits, 8 of 16, 4 of float): 16 C source bytes
// from whatever byte address they start at (a dense rgb24 row starts at 3 w y), separated in registers (image_unpack_body.hpp: v_perm_b32
// for 8- and 16-bit samples, a choice of registers for float) and stored as ONE 16-byte non-temporal vector to each plane, consecutive
// lanes writing consecutive 16 bytes. A workgroup of 256 lanes takes a band of rows of a frame, as many as fill it once (row_units.hpp).
// Grey (C = 1): the lane loads its 16 bytes itself, one unaligned non-temporal load. Several channels: the workgroup first copies the
// band's bytes, 256 units at a time, into LDS with ALIGNED 16-byte loads, consecutive lanes consecutive chunks, and a lane takes its unit
// from there as 4 C + 1 dwords shifted by the source's byte phase (v_alignbyte_b32). Lanes that load their own units touch 16 bytes of
// every 16 C, which measured 0.58-0.67 of HBM against 0.72-0.80 through LDS; four pixels a lane were slower still.
// BGR / BGRA are RGB / RGBA with the first and third plane exchanged on the host. Grey below 8 bits is the 8-bit grey kernel with a
// mask and a multiplier. INDEXED keeps the palette as one packed dword table in LDS, as color_map.hip does: one gather a pixel.
//
// Paths. A frame whose output bases and pitches (in bytes) are all multiples of 16 takes the unit path for the whole units of a row
// and finishes the row's last pixels one by one; any other frame goes pixel by pixel throughout, with the same bits. The source needs
// no alignment at all on either path. Neither path reads outside the w x pixel-bytes of a source row or writes outside [0, w) x h.
#include <algorithm>
#include <climits>

#include "image_unpack_body.hpp"
#include "row_units.hpp"

namespace {

using image_unpack::UnpackFrame;
constexpr int kThreads = kRowUnitThreads;
static_assert(kThreads == image_unpack::kThreads);

struct UnpackParams : PlaneTable<UnpackFrame> {
    uint32_t mask4, mul;  // grey below 8 bits
};
struct UnpackIndexedParams : PlaneTable<UnpackFrame> {
    uint32_t pal[256];  // r | g << 8 | b << 16 | a << 24
};

#if defined(__HIPCC__)
template <int S>
__global__ __launch_bounds__(kThreads) void image_unpack_grey_kernel(const UnpackParams prm) {
    const int wg = blockIdx.x;
    const UnpackFrame &f = prm.p[vszip_find_plane(prm, wg)];
    image_unpack::grey_lane<S>(f, wg - f.block0, (int)threadIdx.x, prm.mask4, prm.mul);
}

template <int S, int C>
__global__ __launch_bounds__(kThreads) void image_unpack_kernel(const UnpackParams prm) {
    typedef uint32_t Chunk __attribute__((ext_vector_type(4)));
    __shared__ Chunk lds[image_unpack::staged_chunks(C)];
    const int wg = blockIdx.x, tid = (int)threadIdx.x;
    const UnpackFrame &f = prm.p[vszip_find_plane(prm, wg)];
    const image_unpack::Band<S, C> band(f, wg - f.block0);
    const int sweeps = image_unpack::staged_sweeps(band);  // (the same for every lane of the workgroup)
    for (int t = 0; t < sweeps; ++t) {
        if (t > 0) __syncthreads();
        image_unpack::stage_sweep(band, t, tid, reinterpret_cast<uint32_t *>(lds));
        __syncthreads();
        image_unpack::unpack_sweep(band, t, tid, reinterpret_cast<const uint32_t *>(lds));
    }
    image_unpack::staged_tail(band, tid);
}

__global__ __launch_bounds__(kThreads) void image_unpack_indexed_kernel(const UnpackIndexedParams prm) {
    static_assert(kThreads == 256);
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = prm.pal[threadIdx.x];
    __syncthreads();
    const int wg = blockIdx.x;
    const UnpackFrame &f = prm.p[vszip_find_plane(prm, wg)];
    image_unpack::band_lane_indexed(f, wg - f.block0, (int)threadIdx.x, tab);
}
#endif  // __HIPCC__

struct Shape {
    int c, s, g;  // samples a pixel, bytes a sample, pixels a unit
};

// plane i of the table from frame i of the call: o[] in the pixel's memory order
template <typename Table, typename Kernel>
int unpack_run(vszip_ctx *ctx, Table &prm, Kernel kernel, int layout, Shape sh, const vszip_image_unpack_frame *frames, int nframes) {
    return vszip_for_each_table(
        ctx, prm, nframes,
        [&](UnpackFrame &d, int i) -> int {
            const vszip_image_unpack_frame &s = frames[i];
            const bool grey = layout == VSZIP_IMG_GRAY || layout == VSZIP_IMG_GRAY_ALPHA, bgr = layout == VSZIP_IMG_BGR || layout == VSZIP_IMG_BGRA;
            const int colour = grey ? 1 : 3, nout = layout == VSZIP_IMG_INDEXED ? 4 : sh.c;
            d.src = static_cast<const uint8_t *>(s.src);
            d.ss = (int)s.src_stride;
            for (int c = 0; c < 4; ++c) d.o[c] = nullptr, d.os[c] = 0;
            for (int c = 0; c < colour; ++c) {
                const int k = bgr ? 2 - c : c;
                d.o[c] = s.p[k];
                d.os[c] = (int)s.p_stride[k];
            }
            if (nout > colour && s.a) d.o[colour] = s.a, d.os[colour] = (int)s.a_stride;
            d.w = s.w;
            d.h = s.h;
            uintptr_t bits = 0;
            for (int c = 0; c < 4; ++c)
                if (d.o[c]) bits |= reinterpret_cast<uintptr_t>(d.o[c]) | (uintptr_t)((size_t)d.os[c] * sh.s);
            d.vec = (bits & 15) == 0;
            d.rows = (short)vszip_rows_per_workgroup(d.vec ? s.w / sh.g : s.w);
            return (s.h + d.rows - 1) / d.rows;
        },
        [&](const Table &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}

const char *const kLayoutName[] = {"GRAY", "GRAY_ALPHA", "RGB", "RGBA", "BGR", "BGRA", "INDEXED"};

}  // namespace

VSZIP_EXPORT int vszip_image_unpack(vszip_ctx *ctx, int layout, int dtype, int src_bits, const vszip_image_unpack_frame *frames, int nframes, const uint8_t palette[256][4]) {
    if (!ctx || !frames || nframes <= 0) return VSZIP_ERR_ARG;
    if (layout < VSZIP_IMG_GRAY || layout > VSZIP_IMG_INDEXED) return vszip_set_error(ctx, VSZIP_ERR_ARG, "ImageUnpack: layout %d is not one of VSZIP_IMG_GRAY .. VSZIP_IMG_INDEXED", layout);
    if (layout == VSZIP_IMG_INDEXED && (src_bits != 8 || dtype != VSZIP_U8))
        return vszip_set_error(ctx, VSZIP_ERR_ARG, "ImageUnpack: INDEXED takes one 8-bit index a pixel and gives 8-bit planes, not an index width of %d (indexed16 is not served) or type %d", src_bits, dtype);
    const bool grey = layout == VSZIP_IMG_GRAY || layout == VSZIP_IMG_GRAY_ALPHA, alpha = layout == VSZIP_IMG_GRAY_ALPHA || layout == VSZIP_IMG_RGBA || layout == VSZIP_IMG_BGRA || layout == VSZIP_IMG_INDEXED;
    const bool bgr = layout == VSZIP_IMG_BGR || layout == VSZIP_IMG_BGRA;
    // the combinations of the reference's switch (image_read.zig:285-345) and no others
    bool served;
    if (dtype == VSZIP_U8)
        served = src_bits == 8 || (layout == VSZIP_IMG_GRAY && (src_bits == 1 || src_bits == 2 || src_bits == 4));
    else if (dtype == VSZIP_U16)
        served = src_bits == 16 && !bgr;
    else
        served = dtype == VSZIP_F32 && src_bits == 32 && layout == VSZIP_IMG_RGBA;
    if (!served) return vszip_set_error(ctx, VSZIP_ERR_ARG, "ImageUnpack: %s with type %d and %d source bits is not served", kLayoutName[layout], dtype, src_bits);
    if ((layout == VSZIP_IMG_INDEXED) != (palette != nullptr))
        return vszip_set_error(ctx, VSZIP_ERR_ARG, layout == VSZIP_IMG_INDEXED ? "ImageUnpack: INDEXED needs a palette" : "ImageUnpack: palette must be NULL for %s", kLayoutName[layout]);
    const Shape sh = {layout == VSZIP_IMG_INDEXED ? 1 : (grey ? 1 : 3) + (alpha ? 1 : 0), dtype == VSZIP_U8 ? 1 : dtype == VSZIP_U16 ? 2 : 4, dtype == VSZIP_U8 ? 16 : dtype == VSZIP_U16 ? 8 : 4};
    const int colour = grey ? 1 : 3;
    long long rows = 0;
    for (int i = 0; i < nframes; ++i) {
        const vszip_image_unpack_frame &s = frames[i];
        bool null = !s.src;
        for (int c = 0; c < colour; ++c) null |= !s.p[c];
        if (null) return vszip_set_error(ctx, VSZIP_ERR_ARG, grey ? "ImageUnpack: frame %d: src and p[0] must not be NULL" : "ImageUnpack: frame %d: src, p[0], p[1] and p[2] must not be NULL", i);
        ptrdiff_t lo = PTRDIFF_MAX, hi = 0;
        for (int c = 0; c < colour; ++c) lo = std::min(lo, s.p_stride[c]), hi = std::max(hi, s.p_stride[c]);
        if (alpha && s.a) lo = std::min(lo, s.a_stride), hi = std::max(hi, s.a_stride);
        const long long row_bytes = (long long)s.w * sh.c * sh.s;
        if (s.w < 1 || s.h < 1 || lo < s.w || hi > INT_MAX || s.src_stride < row_bytes || s.src_stride > INT_MAX)
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "ImageUnpack: frame %d: bad geometry %dx%d, source pitch %lld bytes for rows of %lld, plane pitches %lld .. %lld", i, (int)s.w,
                                   (int)s.h, (long long)s.src_stride, row_bytes, (long long)lo, (long long)hi);
        rows += s.h;
    }
    if (rows > INT_MAX / 2) return vszip_set_error(ctx, VSZIP_ERR_UNSUPPORTED, "ImageUnpack: %lld rows are more than one call numbers", rows);
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (layout == VSZIP_IMG_INDEXED) {
        UnpackIndexedParams prm;  // the palette is copied into the kernel argument: the caller's array is free when the call returns
        for (int i = 0; i < 256; ++i) prm.pal[i] = (uint32_t)palette[i][0] | ((uint32_t)palette[i][1] << 8) | ((uint32_t)palette[i][2] << 16) | ((uint32_t)palette[i][3] << 24);
        return unpack_run(ctx, prm, image_unpack_indexed_kernel, layout, sh, frames, nframes);
    }
    UnpackParams prm;
    const uint32_t m = (1u << std::min(src_bits, 8)) - 1u;
    prm.mask4 = m * 0x01010101u;
    prm.mul = 255u / m;
    void (*kernel)(const UnpackParams) = nullptr;
    switch (sh.s * 10 + sh.c) {
        case 11: kernel = image_unpack_grey_kernel<1>; break;
        case 21: kernel = image_unpack_grey_kernel<2>; break;
        case 12: kernel = image_unpack_kernel<1, 2>; break;
        case 13: kernel = image_unpack_kernel<1, 3>; break;
        case 14: kernel = image_unpack_kernel<1, 4>; break;
        case 22: kernel = image_unpack_kernel<2, 2>; break;
        case 23: kernel = image_unpack_kernel<2, 3>; break;
        case 24: kernel = image_unpack_kernel<2, 4>; break;
        default: kernel = image_unpack_kernel<4, 4>; break;
    }
    return unpack_run(ctx, prm, kernel, layout, sh, frames, nframes);
}
