// vszip.AdaptiveBinarize on gfx950 (src/vapoursynth/adaptive_binarize.zig:26-73): 8-bit planes,
// dst = 255 where clip2 - clip >= c (compared in i16), else 0. Two streams in, one out, 16 bytes
// per lane; one launch per table of planes.
#include <algorithm>

#include "plane_table.hpp"

namespace {

typedef StreamPlane<2> ABPlane;  // in[]: clip, clip2
struct ABParams : PlaneTable<ABPlane> {
    int c;
};

struct AdaptiveBinarizeOp {
    static constexpr int kInputs = 2, kRows = 4;
    static constexpr bool kNontemporalLoads = false, kLastMayAlias = false;
    static __device__ __forceinline__ uint8_t f(const uint8_t (&px)[2], StreamNoExtra, const ABParams &prm) { return ((int)px[1] - (int)px[0] >= prm.c) ? 255 : 0; }
};

__global__ __launch_bounds__(256) void adaptive_binarize_kernel(const ABParams prm) {
    stream_map_rows<uint8_t, AdaptiveBinarizeOp>(prm);
}

}  // namespace

VSZIP_EXPORT int vszip_adaptive_binarize(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, int c) {
    if (!ctx || !planes || nplanes <= 0) return VSZIP_ERR_ARG;
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ABParams prm;
    prm.c = std::min(std::max(c, -256), 256);  // :96-99
    return stream_map_run<AdaptiveBinarizeOp>(ctx, prm, nplanes, adaptive_binarize_kernel, [&](ABPlane &d, int i) -> int {
        const vszip_plane &s = planes[i];
        if (!s.src || !s.ref || !s.dst || s.w <= 0 || s.h <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "AdaptiveBinarize: bad plane %d", i);
        d.in[0] = s.src;
        d.in[1] = s.ref;
        d.dst = s.dst;
        d.istride[0] = (int)s.src_stride;
        d.istride[1] = (int)s.ref_stride;
        d.dstride = (int)s.dst_stride;
        d.w = s.w;
        d.h = s.h;
        return VSZIP_OK;
    });
}
