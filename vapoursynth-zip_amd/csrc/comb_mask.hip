// vszip.CombMask and vszip.CombMaskMT on gfx950 (src/filters/comb_mask.zig, src/filters/comb_mask_mt.zig): 8-bit planes,
// a vertical 5- or 3-row comb metric with mirrored edge rows, optionally gated by a temporal difference that is dilated
// over three rows, optionally dilated over three columns. One pass, one launch per table of planes: every variant reads
// each input sample about once and writes each output sample once; no mask or difference plane goes to memory.
//
// Work layout. A wave owns kBandRows rows of a strip of columns and walks down them with the rows it needs in registers
// (five source rows, three rows of the motion mask), one new row of each input per step, loaded one step ahead. A lane
// holds 16 samples of a row, as 16-bit lanes of eight registers, so that the metric runs on packed 16-bit instructions
// (two samples each) without compares: x > y is "x -sat y != 0"; masks are a flag byte per sample until the store. With expansion the first and the last lane of a wave
// compute a lane group they do not store (62 of 64 lane groups are output), so the gated mask left and right of every
// stored group comes from the neighbouring lane and no wave needs another wave's result. The four waves of a workgroup
// take consecutive strips, then the next band: a workgroup owns a band of rows of its plane.
//
// Paths. 16-byte loads and stores need 16-byte aligned bases and pitches of every plane of the entry; any other plane
// runs the same code on byte loads and byte stores. Only [0, w) x h is written; a 16-byte load of the last lane group may
// cover pitch padding (inside h x stride), whose only possible effect is on the expansion of column w - 1, which is
// never expanded.
#include <algorithm>

#include "plane_table.hpp"

namespace {

constexpr int kBandRows = 16;  // rows a wave produces; it loads 4 (metric 0) or 2 more source rows and 2 more of the previous frame

struct CombPlane {
    const uint8_t *src, *prv;
    uint8_t *dst;
    int sstride, pstride, dstride, w, h;
    int strips;  // waves side by side
    int block0;
};
struct CombParams : PlaneTable<CombPlane> {
    int thr;       // cthresh, or thY2
    int thr6;      // 6 * cthresh (metric 0)
    int mthresh;   // motion
    int thy1;      // CombMaskMT with thY1 < thY2 ...
    uint32_t inv;  // ... and floor(2^32 / (thY2 - thY1)) + 1: n * inv >> 32 == n / (thY2 - thY1) for n <= 255 * 256
};

enum { kMetric0 = 0, kMetric1 = 1, kMtBinary = 2, kMtGradient = 3 };

#if defined(__HIPCC__)
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct Row {
    us2 v[8];  // v[2k]: bytes 0 and 2 of dword k, v[2k + 1]: bytes 1 and 3
};

__device__ __forceinline__ us2 as_us2(uint32_t x) { return __builtin_bit_cast(us2, x); }
__device__ __forceinline__ uint32_t as_u32(us2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ us2 splat(int v) { return us2{(unsigned short)v, (unsigned short)v}; }
__device__ __forceinline__ us2 sat_sub(us2 a, us2 b) { return __builtin_elementwise_sub_sat(a, b); }
__device__ __forceinline__ us2 vmin(us2 a, us2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ us2 vmax(us2 a, us2 b) { return __builtin_elementwise_max(a, b); }

__device__ __forceinline__ Row unpack(u4 r) {
    Row o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o.v[2 * k] = as_us2(r[k] & 0x00FF00FFu);
        o.v[2 * k + 1] = as_us2((r[k] >> 8) & 0x00FF00FFu);
    }
    return o;
}

// Flags: a dword of four bytes 0 / 1, one per sample. 1 in every byte whose 16-bit lane (even: bytes 0 and 2, odd: bytes 1
// and 3) is not zero: x +sat 0xFFFE is odd exactly for x != 0 (written so because min(x, 1) is compiled to a compare and a
// select per sample).
__device__ __forceinline__ uint32_t flags_nonzero(us2 even, us2 odd) {
    const uint32_t e = as_u32(__builtin_elementwise_add_sat(even, splat(0xFFFE))) & 0x00010001u;
    const uint32_t o = as_u32(__builtin_elementwise_add_sat(odd, splat(0xFFFE))) & 0x00010001u;
    return e | (o << 8);
}
__device__ __forceinline__ uint32_t flags_to_mask(uint32_t z) { return (z << 8) - z; }  // 1 -> 0xFF in every byte

// max((b - c) * (d - c), 0): at most one of the two products is not zero, and 255 * 255 fits 16 bits
__device__ __forceinline__ us2 comb_product(us2 b, us2 c, us2 d) { return sat_sub(b, c) * sat_sub(d, c) + sat_sub(c, b) * sat_sub(c, d); }

template <int Mode>
__device__ __forceinline__ us2 metric(const Row *win, int i, const CombParams &prm) {
    if constexpr (Mode == kMetric0) {
        const us2 a = win[0].v[i], b = win[1].v[i], c = win[2].v[i], d = win[3].v[i], e = win[4].v[i];
        const us2 t = splat(prm.thr), t6 = splat(prm.thr6);
        // c - b > t and c - d > t, or b - c > t and d - c > t
        const us2 c1 = sat_sub(c, vmax(b, d) + t) | sat_sub(vmin(b, d), c + t);
        const us2 s1 = a + e + c * splat(4), s2 = (b + d) * splat(3);
        const us2 c2 = sat_sub(s1, s2 + t6) | sat_sub(s2, s1 + t6);  // |s1 - s2| > 6 t
        return vmin(c1, c2);                                         // both
    } else {
        return sat_sub(comb_product(win[0].v[i], win[1].v[i], win[2].v[i]), splat(prm.thr));
    }
}

__device__ __forceinline__ uint32_t mt_gradient(uint32_t p, const CombParams &prm) {
    const uint32_t g = std::min(__umulhi((p - (uint32_t)prm.thy1) << 8, prm.inv), 255u);
    return (int)p < prm.thy1 ? 0u : ((int)p > prm.thr ? 255u : g);
}

// the 16 samples of the window's centre row: flags, or (kMtGradient) the output bytes themselves
template <int Mode>
__device__ __forceinline__ u4 spatial_mask(const Row *win, const CombParams &prm) {
    u4 m;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (Mode == kMtGradient) {
            const us2 e = comb_product(win[0].v[2 * k], win[1].v[2 * k], win[2].v[2 * k]);
            const us2 o = comb_product(win[0].v[2 * k + 1], win[1].v[2 * k + 1], win[2].v[2 * k + 1]);
            m[k] = mt_gradient(e.x, prm) | (mt_gradient(o.x, prm) << 8) | (mt_gradient(e.y, prm) << 16) | (mt_gradient(o.y, prm) << 24);
        } else {
            m[k] = flags_nonzero(metric<Mode>(win, 2 * k, prm), metric<Mode>(win, 2 * k + 1, prm));
        }
    }
    return m;
}

// |src - prv| > mthresh, as flags
__device__ __forceinline__ u4 motion_mask(const Row &s, u4 prv, const CombParams &prm) {
    const Row p = unpack(prv);
    const us2 t = splat(prm.mthresh);
    us2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = sat_sub(sat_sub(s.v[i], p.v[i]) | sat_sub(p.v[i], s.v[i]), t);
    u4 m;
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = flags_nonzero(v[2 * k], v[2 * k + 1]);
    return m;
}

// 16 samples from x0 of a row; samples at and beyond w read as 0 on the byte path
template <bool Vec>
__device__ __forceinline__ u4 load_group(const uint8_t *row, int x0, int w) {
    if constexpr (Vec) {
        return stream_load<true>(reinterpret_cast<const u4 *>(row + x0));  // every sample is read once (band halos aside)
    } else {
        u4 r = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (x0 + k < w) r[k >> 2] |= (uint32_t)row[x0 + k] << (8 * (k & 3));
        return r;
    }
}

template <int Mode, bool Expand, bool Motion, bool Vec>
__device__ __forceinline__ void comb_band(const CombPlane &pl, const CombParams &prm, int y0, int y1, int x0, bool stores) {
    constexpr int W = Mode == kMetric0 ? 5 : 3, C = W / 2;
    const int w = pl.w, h = pl.h;
    const bool active = x0 >= 0 && x0 < w;
    const u4 zero = {0, 0, 0, 0};
    auto src_row = [&](int y) -> u4 {  // mirrored without repeating the edge row; h >= 3
        y = y < 0 ? -y : (y >= h ? 2 * (h - 1) - y : y);
        return active ? load_group<Vec>(pl.src + (size_t)y * pl.sstride, x0, w) : zero;
    };
    auto prv_row = [&](int y) -> u4 { return active ? load_group<Vec>(pl.prv + (size_t)y * pl.pstride, x0, w) : zero; };  // 0 <= y < h

    Row win[W];     // after a step's shift: rows y - C .. y + C
    u4 mo[3] = {zero, zero, zero};  // motion of rows y - 1, y, y + 1 (0 outside the plane)
#pragma unroll
    for (int k = 1; k < W; ++k) win[k] = unpack(src_row(y0 - C + k - 1));
    if constexpr (Motion) {
        if (y0 > 0) mo[1] = motion_mask(win[C], prv_row(y0 - 1), prm);
        mo[2] = motion_mask(win[C + 1], prv_row(y0), prm);
    }
    u4 next_s = src_row(y0 + C), next_p = zero;
    if constexpr (Motion)
        if (y0 + 1 < h) next_p = prv_row(y0 + 1);

    for (int y = y0; y < y1; ++y) {
        const u4 cur_s = next_s, cur_p = next_p;
        if (y + 1 < y1) {  // the next step's rows, before this step's arithmetic
            next_s = src_row(y + 1 + C);
            if constexpr (Motion)
                if (y + 2 < h) next_p = prv_row(y + 2);
        }
#pragma unroll
        for (int k = 0; k + 1 < W; ++k) win[k] = win[k + 1];
        win[W - 1] = unpack(cur_s);
        u4 m = spatial_mask<Mode>(win, prm);
        if constexpr (Mode >= kMtBinary)
            if (y == 0 || y == h - 1) m = zero;
        if constexpr (Motion) {
            mo[0] = mo[1];
            mo[1] = mo[2];
            mo[2] = y + 1 < h ? motion_mask(win[C + 1], cur_p, prm) : zero;
            m &= mo[0] | mo[1] | mo[2];
        }
        if (!active) m = zero;
        u4 o = m;
        if constexpr (Expand) {
            // the gated mask one column left and right: across dwords, and across lanes for the first and last column
            const uint32_t left = __shfl_up(m[3], 1, 64), right = __shfl_down(m[0], 1, 64);
            o[0] |= (m[0] << 8) | (left >> 24);
            o[1] |= (m[1] << 8) | (m[0] >> 24);
            o[2] |= (m[2] << 8) | (m[1] >> 24);
            o[3] |= (m[3] << 8) | (m[2] >> 24);
            o[0] |= (m[0] >> 8) | (m[1] << 24);
            o[1] |= (m[1] >> 8) | (m[2] << 24);
            o[2] |= (m[2] >> 8) | (m[3] << 24);
            o[3] |= (m[3] >> 8) | (right << 24);
            const int last = w - 1 - x0;  // column w - 1 is never expanded
            if (last >= 0 && last < 16) {
                const uint32_t keep = 0xFFu << (8 * (last & 3));
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k == (last >> 2)) o[k] = (o[k] & ~keep) | (m[k] & keep);
            }
        }
        if constexpr (Mode != kMtGradient) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = flags_to_mask(o[k]);
        }
        if (stores && active) {
            uint8_t *d = pl.dst + (size_t)y * pl.dstride + x0;
            if (Vec && x0 + 16 <= w) {
                *reinterpret_cast<u4 *>(d) = o;
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (x0 + k < w) d[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

template <int Mode, bool Expand, bool Motion>
__global__ __launch_bounds__(256) void comb_mask_kernel(const CombParams prm) {
    constexpr int kOut = Expand ? 62 : 64;  // lane groups a wave stores
    const int b = blockIdx.x;
    const CombPlane &pl = prm.p[vszip_find_plane(prm, b)];
    const int unit = (b - pl.block0) * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int band = unit / pl.strips, strip = unit - band * pl.strips;
    const int y0 = band * kBandRows;
    if (y0 >= pl.h) return;  // (no barrier below)
    const int y1 = std::min(y0 + kBandRows, pl.h);
    const int x0 = (strip * kOut + lane - (Expand ? 1 : 0)) * 16;
    const bool stores = !Expand || (lane >= 1 && lane <= 62);
    uintptr_t bits = reinterpret_cast<uintptr_t>(pl.src) | (uintptr_t)pl.sstride | reinterpret_cast<uintptr_t>(pl.dst) | (uintptr_t)pl.dstride;
    if (Motion) bits |= reinterpret_cast<uintptr_t>(pl.prv) | (uintptr_t)pl.pstride;
    if ((bits & 15) == 0)
        comb_band<Mode, Expand, Motion, true>(pl, prm, y0, y1, x0, stores);
    else
        comb_band<Mode, Expand, Motion, false>(pl, prm, y0, y1, x0, stores);
}
#endif  // __HIPCC__

typedef void (*CombKernel)(const CombParams);

// planes -> tables -> launches of `kernel`; expand: the waves keep a lane group of apron on either side
int comb_run(vszip_ctx *ctx, CombParams &prm, const vszip_plane *planes, int nplanes, bool motion, bool expand, CombKernel kernel) {
    const int out_groups = expand ? 62 : 64;
    return vszip_for_each_table(
        ctx, prm, nplanes,
        [&](CombPlane &d, int i) -> int {
            const vszip_plane &s = planes[i];
            d.src = static_cast<const uint8_t *>(s.src);
            d.prv = motion ? static_cast<const uint8_t *>(s.ref) : d.src;
            d.dst = static_cast<uint8_t *>(s.dst);
            d.sstride = (int)s.src_stride;
            d.pstride = motion ? (int)s.ref_stride : d.sstride;
            d.dstride = (int)s.dst_stride;
            d.w = s.w;
            d.h = s.h;
            d.strips = ((s.w + 15) / 16 + out_groups - 1) / out_groups;
            const int bands = (s.h + kBandRows - 1) / kBandRows;
            return (d.strips * bands + 3) / 4;
        },
        [&](const CombParams &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}

int check_planes(vszip_ctx *ctx, const char *name, const vszip_plane *planes, int nplanes, bool need_ref) {
    for (int i = 0; i < nplanes; ++i) {
        const vszip_plane &s = planes[i];
        if (!s.src || !s.dst) return vszip_set_error(ctx, VSZIP_ERR_ARG, "%s: plane %d: src and dst must not be NULL", name, i);
        if (need_ref && !s.ref) return vszip_set_error(ctx, VSZIP_ERR_ARG, "%s: plane %d: ref (the previous frame's plane) must not be NULL when mthresh > 0", name, i);
        if (s.w <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "%s: bad plane %d", name, i);
        if (s.h < 3) return vszip_set_error(ctx, VSZIP_ERR_ARG, "%s: clip too small; every plane must be at least 3 rows tall.", name);
    }
    return VSZIP_OK;
}

}  // namespace

VSZIP_EXPORT int vszip_comb_mask(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, int cthresh, int mthresh, int expand, int metric) {
    if (!ctx || !planes || nplanes <= 0) return VSZIP_ERR_ARG;
    // combMaskCreate, src/vapoursynth/comb_mask.zig:93-120
    const int cth_max = metric ? 65025 : 255;
    if (cthresh > cth_max || cthresh < 0)
        return vszip_set_error(ctx, VSZIP_ERR_ARG, "CombMask: cthresh must be between 0 and %d when metric = %s.", cth_max, metric ? "true" : "false");
    if (mthresh > 255 || mthresh < 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "CombMask: mthresh must be between 0 and 255.");
    const bool motion = mthresh > 0;
    const int rc = check_planes(ctx, "CombMask", planes, nplanes, motion);
    if (rc != VSZIP_OK) return rc;
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    CombParams prm;
    prm.thr = cthresh;
    prm.thr6 = 6 * cthresh;
    prm.mthresh = mthresh;
    prm.thy1 = 0;
    prm.inv = 0;
    // the reference's eight getFrame variants (:133-146)
    static const CombKernel kernels[2][2][2] = {
        {{comb_mask_kernel<kMetric0, false, false>, comb_mask_kernel<kMetric0, false, true>},
         {comb_mask_kernel<kMetric0, true, false>, comb_mask_kernel<kMetric0, true, true>}},
        {{comb_mask_kernel<kMetric1, false, false>, comb_mask_kernel<kMetric1, false, true>},
         {comb_mask_kernel<kMetric1, true, false>, comb_mask_kernel<kMetric1, true, true>}}};
    return comb_run(ctx, prm, planes, nplanes, motion, expand != 0, kernels[metric ? 1 : 0][expand ? 1 : 0][motion ? 1 : 0]);
}

VSZIP_EXPORT int vszip_comb_mask_mt(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, int thy1, int thy2) {
    if (!ctx || !planes || nplanes <= 0) return VSZIP_ERR_ARG;
    // combMaskMTCreate, src/vapoursynth/comb_mask_mt.zig:87-110
    if (thy1 > 255 || thy1 < 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "CombMaskMT: thY1 value should be in range [0;255]");
    if (thy2 > 255 || thy2 < 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "CombMaskMT: thY2 value should be in range [0;255]");
    if (thy1 > thy2) return vszip_set_error(ctx, VSZIP_ERR_ARG, "CombMaskMT: thY1 can't be greater than thY2");
    const int rc = check_planes(ctx, "CombMaskMT", planes, nplanes, false);
    if (rc != VSZIP_OK) return rc;
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    CombParams prm;
    prm.thr = thy2;
    prm.thr6 = 0;
    prm.mthresh = 0;
    prm.thy1 = thy1;
    prm.inv = thy1 == thy2 ? 0u : (thy2 - thy1 == 1 ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / (uint32_t)(thy2 - thy1)) + 1u);  // (n * (2^32 - 1) >> 32 == min(n, 255) for n in {0, 256})
    return comb_run(ctx, prm, planes, nplanes, false, false,
                    thy1 == thy2 ? comb_mask_kernel<kMtBinary, false, false> : comb_mask_kernel<kMtGradient, false, false>);
}
