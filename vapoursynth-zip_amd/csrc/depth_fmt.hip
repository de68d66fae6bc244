// vszip_depth_fmt on gfx950: the change of sample type that zimg's resize.Point(format=...) makes on the host, between integer (8, 9..16 bits),
// half and float planes. The arithmetic is depth_fmt.hpp's (int_to_float / float_to_int_none, one fused multiply-add each) and, for the error
// diffusion, depth_plan.hpp's diffuse on a float sample with scale = range. Integer -> integer calls are vszip_depth itself.
//
// none. One streaming pass like depth_none_kernel's: a lane owns 16 bytes of the narrower plane and moves the wider side as one or two 16-byte
// accesses (u8 <-> f32: eight samples, 8 bytes and two 16-byte accesses; fmt_lane_samples says why not sixteen); loads are non-temporal (every
// sample is read once), stores as depth_none_kernel makes them;
// a workgroup takes a band of rows in raster order (row_units.hpp). Planes whose bases or pitches (in bytes) are no multiples of 16 go sample by
// sample with the same bits. Half samples are converted by the hardware's conversions: nearest even, subnormals kept.
//
// error diffusion. depth.hip's wavefront kernel, instantiated here for f32 and f16 sources (this object holds fused multiply-adds, depth.o must
// not: tests/test_depth_isa.py): Group<float> is eight dwords filled by two 16-byte loads, Group<_Float16> rides the 16-bit form and widens at
// pop. Served where the offset is 0 (full range, non-chroma), so the sample's scaled value is the plain product diffuse() makes.
#define VSZIP_DEPTH_KERNELS_ONLY
#include "depth.hip"
#include "depth_fmt.hpp"

namespace {

namespace df = depth_fmt;

// An entry is 48 bytes; 128 of them are 6 KiB of kernel argument.
constexpr int kFmtPlanes = 128;
struct FmtPlane {
    const void *src;
    void *dst;
    int sstride, dstride, w, h;
    float a, b;  // int -> float: mul, add; float -> int: range, offset (the plane's: chroma differs from luma)
    short vec;   // both bases and pitches are multiples of 16 bytes
    short rows;  // rows a workgroup
    int block0;
};
struct FmtParams : PlaneTable<FmtPlane, kFmtPlanes> {
    float peak;  // float -> int: 2^bits_out - 1
};

// Samples a lane: 16 bytes of the narrower plane, but no more than 32 of the wider one. u8 <-> f32 at sixteen samples a lane made every store
// instruction of a wave write 16 bytes in every 64 (four instructions to fill a line): 1.5 TB/s against 5 for the two-access shape.
template <typename Tin, typename Tout>
constexpr int fmt_lane_samples() {
    constexpr int narrow = sizeof(Tin) < sizeof(Tout) ? sizeof(Tin) : sizeof(Tout), wide = sizeof(Tin) < sizeof(Tout) ? sizeof(Tout) : sizeof(Tin);
    return 16 / narrow < 32 / wide ? 16 / narrow : 32 / wide;
}

#if defined(__HIPCC__)
template <typename Tin, typename Tout>
__device__ __forceinline__ Tout fmt_convert(Tin v, float a, float b, float peak) {
    if constexpr (std::is_integral_v<Tin>) {
        float f = df::int_to_float((float)v, a, b);
        // to half: the f32 result is rounded once more. The empty asm keeps the two roundings apart: LLVM folds fma + conversion into
        // v_fma_mixlo_f16, which rounds the exact sum to half ONCE and differs in the last bit of some samples
        if constexpr (sizeof(Tout) == 2) asm("" : "+v"(f));
        return (Tout)f;
    } else if constexpr (std::is_integral_v<Tout>)
        return (Tout)df::float_to_int_none((float)v, a, b, peak);  // (from half: widened, exact)
    else
        return (Tout)(float)v;
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(kRowUnitThreads) void depth_fmt_none_kernel(const FmtParams prm) {
    constexpr int V = fmt_lane_samples<Tin, Tout>();
    typedef Tin VI __attribute__((ext_vector_type(V), aligned(V * sizeof(Tin) < 16 ? V * sizeof(Tin) : 16)));
    typedef Tout VO __attribute__((ext_vector_type(V), aligned(V * sizeof(Tout) < 16 ? V * sizeof(Tout) : 16)));
    const int wg = blockIdx.x;
    const FmtPlane &f = prm.p[vszip_find_plane(prm, wg)];
    const int y0 = (wg - f.block0) * f.rows, rows = min((int)f.rows, f.h - y0), w = f.w, ss = f.sstride, ds = f.dstride;
    const Tin *s = static_cast<const Tin *>(f.src) + (size_t)y0 * ss;
    Tout *d = static_cast<Tout *>(f.dst) + (size_t)y0 * ds;
    const float a = f.a, b = f.b, peak = prm.peak;
    int x0 = 0;
    if (f.vec) {
        const int nv = w / V;
        for_each_row_unit(rows, nv, [&](int row, int i) {
            const VI v = __builtin_nontemporal_load(reinterpret_cast<const VI *>(s + (size_t)row * ss) + i);
            VO o;
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = fmt_convert<Tin, Tout>(v[e], a, b, peak);
            __builtin_nontemporal_store(o, reinterpret_cast<VO *>(d + (size_t)row * ds) + i);
        });
        x0 = nv * V;
    }
    for_each_row_unit(rows, w - x0, [&](int row, int i) {
        const size_t x = (size_t)x0 + i;
        d[(size_t)row * ds + x] = fmt_convert<Tin, Tout>(s[(size_t)row * ss + x], a, b, peak);
    });
}
#endif  // __HIPCC__

struct FmtCall {
    int bits_in, bits_out, full_range;
    bool in_float, out_float;
};

template <typename Tin, typename Tout>
int fmt_none(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, const FmtCall &c) {
    FmtParams prm;
    prm.peak = c.out_float ? 0.0f : (float)((1u << c.bits_out) - 1u);
    constexpr int V = fmt_lane_samples<Tin, Tout>();
    return vszip_for_each_table(
        ctx, prm, nplanes,
        [&](FmtPlane &d, int i) -> int {
            const vszip_depth_plane &s = planes[i];
            d.src = s.src;
            d.dst = s.dst;
            d.sstride = (int)s.src_stride;
            d.dstride = (int)s.dst_stride;
            d.w = s.w;
            d.h = s.h;
            d.a = d.b = 0.0f;
            if (!c.in_float) {
                const df::ToFloat t = df::to_float_of(df::range_of(c.bits_in, c.full_range != 0, s.chroma != 0));
                d.a = t.mul, d.b = t.add;
            } else if (!c.out_float) {
                const df::Range r = df::range_of(c.bits_out, c.full_range != 0, s.chroma != 0);
                d.a = (float)r.rng, d.b = (float)r.off;
            }
            d.vec = aligned16(s.src, s.src_stride, sizeof(Tin)) && aligned16(s.dst, s.dst_stride, sizeof(Tout));
            d.rows = (short)vszip_rows_per_workgroup(d.vec ? s.w / V : s.w);
            return (s.h + d.rows - 1) / d.rows;
        },
        [&](const FmtParams &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            hipLaunchKernelGGL((depth_fmt_none_kernel<Tin, Tout>), dim3(blocks), dim3(kRowUnitThreads), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}

template <typename Tin>
int fmt_none_from(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, int dtype_out, const FmtCall &c) {
    if constexpr (!std::is_integral_v<Tin>) {  // (integer -> integer is vszip_depth's)
        if (dtype_out == df::kU8) return fmt_none<Tin, uint8_t>(ctx, planes, nplanes, c);
        if (dtype_out == df::kU16) return fmt_none<Tin, uint16_t>(ctx, planes, nplanes, c);
    }
    return dtype_out == df::kF16 ? fmt_none<Tin, _Float16>(ctx, planes, nplanes, c) : fmt_none<Tin, float>(ctx, planes, nplanes, c);
}

// error diffusion from a float plane: the planes of either workgroup size through theirs, as vszip_depth_queue sends the integer ones
template <typename Tin, typename Tout>
int fmt_diffuse(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, const FmtCall &c, const std::vector<scratch::Region<float>> &carry, char *base) {
    DepthParams prm;
    prm.scale = (float)df::range_of(c.bits_out, true, false).rng;
    prm.peak = (float)((1u << c.bits_out) - 1u);
    std::vector<int> idx[2];
    for (int i = 0; i < nplanes; ++i) idx[vszip_depth_waves(ctx, planes[i].h) == dp::kWavesLarge].push_back(i);
    for (int k = 0; k < 2; ++k) {
        if (idx[k].empty()) continue;
        const int waves = k ? dp::kWavesLarge : dp::kWavesSmall;
        const int rc = vszip_for_each_table(
            ctx, prm, (int)idx[k].size(),
            [&](DepthPlane &d, int j) -> int {
                const int i = idx[k][j];
                depth_fill<Tin, Tout>(d, planes[i], carry[i].count ? carry[i].in(base) : nullptr);
                return 1;
            },
            [&](const DepthParams &t, int blocks, int) {
                vszip_probe_scope probe(ctx);
                launch_diffuse<Tin, Tout>(ctx, waves, blocks, t);
                return VSZIP_OK;
            });
        if (rc != VSZIP_OK) return rc;
    }
    return VSZIP_OK;
}

}  // namespace

VSZIP_EXPORT int vszip_depth_fmt(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, int dtype_in, int bits_in, int dtype_out, int bits_out, int dither,
                                 int full_range) {
    if (!ctx) return VSZIP_ERR_ARG;
    char msg[256];
    const int bad = vszip_depth_fmt_check(dtype_in, bits_in, dtype_out, bits_out, dither, full_range, planes, nplanes, msg, sizeof msg);
    if (bad != VSZIP_OK) return vszip_set_error(ctx, bad, "%s", msg);
    const FmtCall c = {bits_in, bits_out, full_range, df::is_float(dtype_in), df::is_float(dtype_out)};
    if (!c.in_float && !c.out_float) return vszip_depth(ctx, planes, nplanes, bits_in, bits_out, dither, full_range);  // the same code path
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!dither) {
        switch (dtype_in) {
            case df::kU8: return fmt_none_from<uint8_t>(ctx, planes, nplanes, dtype_out, c);
            case df::kU16: return fmt_none_from<uint16_t>(ctx, planes, nplanes, dtype_out, c);
            case df::kF16: return fmt_none_from<_Float16>(ctx, planes, nplanes, dtype_out, c);
            default: return fmt_none_from<float>(ctx, planes, nplanes, dtype_out, c);
        }
    }
    // error diffusion: a float source, an integer destination, offset 0 (the check has seen to all three)
    scratch::Layout lay;
    std::vector<scratch::Region<float>> carry;
    vszip_depth_take_carry(ctx, lay, planes, nplanes, dither, carry);
    char *base = nullptr;
    if (lay.bytes()) {
        const int rc = vszip_reserve_scratch(ctx, lay, &base);
        if (rc != VSZIP_OK) return rc;
    }
    if (dtype_in == df::kF32)
        return dtype_out == df::kU8 ? fmt_diffuse<float, uint8_t>(ctx, planes, nplanes, c, carry, base) : fmt_diffuse<float, uint16_t>(ctx, planes, nplanes, c, carry, base);
    return dtype_out == df::kU8 ? fmt_diffuse<_Float16, uint8_t>(ctx, planes, nplanes, c, carry, base) : fmt_diffuse<_Float16, uint16_t>(ctx, planes, nplanes, c, carry, base);
}
