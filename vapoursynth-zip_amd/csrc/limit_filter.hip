// vszip.LimitFilter on gfx950: process() of src/filters/limit_filter.zig:3-34 — per pixel, the
// filtered sample is kept where |flt - ref| <= thr, the source sample is restored where it exceeds
// thr * elast, and blended in between — in plain f32 operations in the reference's order
// (-ffp-contract=off, IEEE division). Three streams in, one out; one launch per table of planes.
#include <algorithm>

#include "plane_table.hpp"

namespace {

struct LFThr {
    float dark_thr, bright_thr, elast;
};
typedef StreamPlane<3, LFThr> LFPlane;  // in[]: filtered, source, reference (the source again where the caller has none)
typedef PlaneTable<LFPlane> LFParams;

template <typename T>
struct LFSmp {
    static constexpr bool is_int = true;
    static __device__ __forceinline__ float f(T v) { return (float)v; }
};
template <>
struct LFSmp<float> {
    static constexpr bool is_int = false;
    static __device__ __forceinline__ float f(float v) { return v; }
};
template <>
struct LFSmp<_Float16> {
    static constexpr bool is_int = false;
    static __device__ __forceinline__ float f(_Float16 v) { return (float)v; }
};

template <typename T>
__device__ __forceinline__ T limit_px(T fv, T sv, T rv, const LFThr &pl) {
    const float sf = LFSmp<T>::f(sv), ff = LFSmp<T>::f(fv), rf = LFSmp<T>::f(rv);
    const float diff_signed = ff - rf, diff_abs = fabsf(diff_signed);
    const float thr1 = diff_signed > 0 ? pl.bright_thr : pl.dark_thr;
    const float thr2 = thr1 * pl.elast;
    float out;
    if (diff_abs <= thr1)
        out = ff;
    else if (diff_abs >= thr2)
        out = sf;
    else
        out = sf + __fdiv_rn((ff - sf) * (thr2 - diff_abs), thr2 - thr1);  // :28
    if constexpr (LFSmp<T>::is_int)
        return (T)truncf(out + 0.5f);
    else
        return (T)out;
}

template <typename T>
struct LimitFilterOp {
    static constexpr int kInputs = 3, kRows = kStreamRows;
    static constexpr bool kNontemporalLoads = true, kLastMayAlias = true;
    static __device__ __forceinline__ T f(const T (&px)[3], const LFThr &thr, const LFParams &) { return limit_px<T>(px[0], px[1], px[2], thr); }
};

template <typename T>
__global__ __launch_bounds__(256) void limit_filter_kernel(const LFParams prm) {
    stream_map_rows<T, LimitFilterOp<T>>(prm);
}

template <typename T>
int run(vszip_ctx *ctx, const vszip_plane *planes, const void *const *refs, const ptrdiff_t *ref_strides, int nplanes, const float *dark, const float *bright,
        const float *elast) {
    LFParams prm;
    return stream_map_run<LimitFilterOp<T>>(ctx, prm, nplanes, limit_filter_kernel<T>, [&](LFPlane &d, int i) -> int {
        const vszip_plane &s = planes[i];
        if (!s.src || !s.ref || !s.dst || s.w <= 0 || s.h <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "LimitFilter: bad plane %d", i);
        const bool has_ref = refs && refs[i];
        d.in[0] = s.src;
        d.in[1] = s.ref;
        d.in[2] = has_ref ? refs[i] : s.ref;
        d.istride[0] = (int)s.src_stride;
        d.istride[1] = (int)s.ref_stride;
        d.istride[2] = has_ref ? (int)ref_strides[i] : (int)s.ref_stride;
        d.dst = s.dst;
        d.dstride = (int)s.dst_stride;
        d.w = s.w;
        d.h = s.h;
        d.x.dark_thr = dark[i];
        d.x.bright_thr = bright[i];
        d.x.elast = elast[i];
        return VSZIP_OK;
    });
}

}  // namespace

VSZIP_EXPORT int vszip_limit_filter(vszip_ctx *ctx, int dtype, const vszip_plane *planes, const void *const *refs, const ptrdiff_t *ref_strides, int nplanes,
                                    const float *dark_thr, const float *bright_thr, const float *elast) {
    if (!ctx || !planes || !dark_thr || !bright_thr || !elast || nplanes <= 0 || (refs && !ref_strides)) return VSZIP_ERR_ARG;
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    switch (dtype) {
        case VSZIP_U8: return run<uint8_t>(ctx, planes, refs, ref_strides, nplanes, dark_thr, bright_thr, elast);
        case VSZIP_U16: return run<uint16_t>(ctx, planes, refs, ref_strides, nplanes, dark_thr, bright_thr, elast);
        case VSZIP_F16: return run<_Float16>(ctx, planes, refs, ref_strides, nplanes, dark_thr, bright_thr, elast);
        case VSZIP_F32: return run<float>(ctx, planes, refs, ref_strides, nplanes, dark_thr, bright_thr, elast);
    }
    return vszip_set_error(ctx, VSZIP_ERR_ARG, "LimitFilter: not supported Int format.");
}
