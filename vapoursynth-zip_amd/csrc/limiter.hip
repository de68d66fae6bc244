// vszip.Limiter on gfx950: dst = min(max(lo, x), hi) per plane (LimiterRT / Limiter getFrame,
// src/vapoursynth/limiter.zig:28-96; the bounds — explicit min/max arrays or the comptime tables of
// src/filters/limiter.zig:66-91 — are resolved by the wrapper). A pure streaming kernel: 16 bytes per
// lane per access, one launch for a whole table of planes; HBM roofline = every byte read once and
// written once.
#include <algorithm>

#include "plane_table.hpp"

namespace {

struct LClip {
    float lo_f, hi_f;      // float clips (already rounded to the sample type's precision by the host for f16)
    uint32_t lo_u, hi_u;   // integer clips
};
typedef StreamPlane<1, LClip> LPlane;
typedef PlaneTable<LPlane> LParams;

template <typename T>
struct LOps;
template <>
struct LOps<uint8_t> {
    static __device__ __forceinline__ uint8_t f(uint8_t v, const LClip &pl) { return (uint8_t)min(max((uint32_t)v, pl.lo_u), pl.hi_u); }
};
template <>
struct LOps<uint16_t> {
    static __device__ __forceinline__ uint16_t f(uint16_t v, const LClip &pl) { return (uint16_t)min(max((uint32_t)v, pl.lo_u), pl.hi_u); }
};
template <>
struct LOps<uint32_t> {
    static __device__ __forceinline__ uint32_t f(uint32_t v, const LClip &pl) { return min(max(v, pl.lo_u), pl.hi_u); }
};
template <>
struct LOps<float> {
    // @max / @min return the non-NaN operand (maxnum / minnum): fmaxf / fminf
    static __device__ __forceinline__ float f(float v, const LClip &pl) { return fminf(fmaxf(pl.lo_f, v), pl.hi_f); }
};
template <>
struct LOps<_Float16> {
    static __device__ __forceinline__ _Float16 f(_Float16 v, const LClip &pl) { return (_Float16)fminf(fmaxf(pl.lo_f, (float)v), pl.hi_f); }
};

template <typename T>
struct LimiterOp {
    static constexpr int kInputs = 1, kRows = kStreamRows;
    static constexpr bool kNontemporalLoads = true, kLastMayAlias = false;
    static __device__ __forceinline__ T f(const T (&px)[1], const LClip &clip, const LParams &) { return LOps<T>::f(px[0], clip); }
};

template <typename T>
__global__ __launch_bounds__(256) void limiter_kernel(const LParams prm) {
    stream_map_rows<T, LimiterOp<T>>(prm);
}

template <typename T>
int run(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, const double *lo, const double *hi) {
    LParams prm;
    return stream_map_run<LimiterOp<T>>(ctx, prm, nplanes, limiter_kernel<T>, [&](LPlane &d, int i) -> int {
        const vszip_plane &s = planes[i];
        if (!s.src || !s.dst || s.w <= 0 || s.h <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Limiter: bad plane %d", i);
        if (lo[i] > hi[i]) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Limiter: min value must be less than or equal to max value.");
        d.in[0] = s.src;
        d.dst = s.dst;
        d.istride[0] = (int)s.src_stride;
        d.dstride = (int)s.dst_stride;
        d.w = s.w;
        d.h = s.h;
        d.x.lo_u = (uint32_t)std::max(0.0, lo[i]);
        d.x.hi_u = (uint32_t)std::max(0.0, hi[i]);
        float lf = (float)lo[i], hf = (float)hi[i];
        if (std::is_same<T, _Float16>::value) {  // the bounds are f16 values (@floatCast / comptime_float -> f16)
            lf = (float)(_Float16)lf;
            hf = (float)(_Float16)hf;
        }
        d.x.lo_f = lf;
        d.x.hi_f = hf;
        return VSZIP_OK;
    });
}

}  // namespace

VSZIP_EXPORT int vszip_limiter(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes, const double *lo, const double *hi) {
    if (!ctx || !planes || !lo || !hi || nplanes <= 0) return VSZIP_ERR_ARG;
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    switch (dtype) {
        case VSZIP_U8: return run<uint8_t>(ctx, planes, nplanes, lo, hi);
        case VSZIP_U16: return run<uint16_t>(ctx, planes, nplanes, lo, hi);
        case VSZIP_U32: return run<uint32_t>(ctx, planes, nplanes, lo, hi);
        case VSZIP_F16: return run<_Float16>(ctx, planes, nplanes, lo, hi);
        case VSZIP_F32: return run<float>(ctx, planes, nplanes, lo, hi);
    }
    return vszip_set_error(ctx, VSZIP_ERR_ARG, "Limiter: not supported Int format.");
}
