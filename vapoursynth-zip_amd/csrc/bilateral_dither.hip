// vszip.BilateralDither on gfx950 (src/filters/bilateral_dither.zig processPlane as called by src/vapoursynth/bilateral_dither.zig):
// per output sample a weighted mean over a (2 r - 1)^2 window, every tap weighted by how close the `ref` (or source) sample is to the
// centre's: wgt = max(min(m - |vr - cen_ref|, wmax), 0), sum_w += wgt, sum = fmaf(v - cen, wgt, sum), taps strictly in the reference's
// order, then cen + sum / max(sum_w, sum_w_min). Dense: all (2 r - 1)^2 taps, rows outer (961 at the default radius). Sub-sampled:
// the K points of one of 23 lists, picked per row and per group of four samples: list (start(y) + (x >> 2)) % 23 with
// start(y) = (LCG^(y+1)(1) >> 8) % 23, which a thread computes by squaring the LCG's affine map (log2(y) steps).
//
// Work split. A workgroup of 256 threads makes a 64 x 16 tile; a thread makes four horizontally adjacent samples (one group of the
// sub-sampled path, so a thread walks one list). Dense rows slide a four-sample register window along the row: one load per four taps,
// so neither LDS nor the memory path is in the way of the ~6 VALU operations a tap costs. Two ways to fetch, same arithmetic:
//   tile    the tile plus a halo of r - 1 samples on every side, already mirrored and widened to f32, is staged in LDS (a second tile
//           for `ref`); the row pitch is odd, so the four rows a wave reads at a stride of four samples fall on different banks. The
//           sub-sampled path turns the plane's 23 K points into tile-linear offsets once per workgroup, in LDS, where they fit beside
//           the tile(s); where they do not (K goes up to 4096) it reads the pairs from global memory.
//   direct  every tap reads global memory with the mirror applied per tap; any radius.
// The tile path needs (64 + 2 (r - 1) | 1) x (16 + 2 (r - 1)) floats, twice with `ref`, within kLdsBudget.
//
// Mirror: i < 0 -> -1 - i, i >= n -> 2 n - 1 - i; r <= w and r <= h, so one reflection serves every tap of a sample inside the plane.
// Lanes beyond the plane's right edge (a partial group) and staged cells nothing reads are clamped into the plane after the reflection,
// so no load ever leaves [0, w) x h. All loads and stores are per sample: every base alignment and pitch takes the same path.
//
// Bounded launches. A call is cut into launches by planes and by row bands (multiples of 16 rows) so that one launch does at most
// kTapsPerLaunch taps; the dense window serves radius <= kMaxDenseRadius.
#include <algorithm>

#include "plane_table.hpp"

namespace {

constexpr int kTW = 64, kTH = 16, kThreads = 256, kLists = 23;
constexpr int kLdsBudget = 48 * 1024;  // bytes of LDS a workgroup may ask for: three workgroups a CU
constexpr int kMaxDenseRadius = 128;
// Taps of one launch at most. Measured tap rates (profiles/bilateral_dither_timing.txt): 6.9-8.0e12 taps/s dense on the tile path, 3.7-6.4e12
// dense direct, 1.9-3.5e12 sub-sampled on the tile path, 0.39-0.92e12 sub-sampled direct (the slowest: float with ref). 2^36 = 6.9e10 taps are
// 9 ms at the fastest rate and 0.18 s at the slowest.
constexpr long long kTapsPerLaunch = 1ll << 36;

struct BdPlane {
    const void *src, *ref;
    void *dst;
    const int16_t *pts;
    int sstride, rstride, dstride, w, h;
    int y0, y1;  // the row band of this entry
    int radius, K, tiles_x;
    float m, wmax, swmin, peak;
    int block0;
};
constexpr int kBdPlanes = 96;  // 96 bytes an entry: 9 KiB of kernel argument, what a Deband launch carries
struct BdParams : PlaneTable<BdPlane, kBdPlanes> {};

__host__ __device__ inline int bd_pitch(int radius) { return (kTW + 2 * (radius - 1)) | 1; }
__host__ __device__ inline int bd_rows(int radius) { return kTH + 2 * (radius - 1); }
__host__ __device__ inline long long bd_tile_bytes(int radius, bool with_ref) { return (long long)bd_pitch(radius) * bd_rows(radius) * 4 * (with_ref ? 2 : 1); }

#if defined(__HIPCC__)
__device__ __forceinline__ int bd_mirror(int i, int n) {
    i = i < 0 ? -1 - i : i;
    i = i >= n ? 2 * n - 1 - i : i;
    return min(max(i, 0), n - 1);  // (only for lanes and staged cells whose value is never used)
}

__device__ __forceinline__ int bd_start(int y) {
    uint32_t A = 1, C = 0, a = 1664525u, c = 1013904223u;
    for (uint32_t n = (uint32_t)y + 1; n; n >>= 1) {
        if (n & 1) {
            A *= a;
            C = C * a + c;
        }
        c *= a + 1;
        a *= a;
    }
    return (int)(((A + C) >> 8) % kLists);
}

// a point as an offset into the staged tile, from the cell of the output; a point outside the window (no list of
// vszip_bilateral_dither_points has one) is clamped into it, so that no table can make a workgroup read outside what it staged
__device__ __forceinline__ int bd_offset(int px, int py, int p, int pitch) {
    px = min(max(px, -p), p);
    py = min(max(py, -p), p);
    return (py + p) * pitch + px + p;
}

struct BdAcc {
    float cen, cen_ref, sum, sum_w;
};

__device__ __forceinline__ void bd_tap(BdAcc &s, float v, float vr, float m, float wmax) {
    const float wgt = fmaxf(fminf(m - fabsf(vr - s.cen_ref), wmax), 0.0f);
    s.sum_w += wgt;
    s.sum = fmaf(v - s.cen, wgt, s.sum);
}

template <typename T>
__device__ __forceinline__ T bd_finish(const BdAcc &s, float swmin, float peak) {
    const float p = s.cen + s.sum / fmaxf(s.sum_w, swmin);
    if constexpr (std::is_same_v<T, float>)
        return p;
    else
        return (T)__builtin_roundf(fmaxf(fminf(p, peak), 0.0f));
}

template <typename T, bool TILE, bool DENSE, bool REF>
__global__ __launch_bounds__(kThreads) void bilateral_dither_kernel(const BdParams prm) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const BdPlane &pl = prm.p[vszip_find_plane(prm, b)];
    const int tile = b - pl.block0, ty = tile / pl.tiles_x, tx = tile - ty * pl.tiles_x;
    const int w = pl.w, h = pl.h, p = pl.radius - 1, K = pl.K;
    const int x0 = tx * kTW, y0 = pl.y0 + ty * kTH;
    const T *src = static_cast<const T *>(pl.src), *ref = static_cast<const T *>(pl.ref);
    const int sstride = pl.sstride, rstride = pl.rstride;
    [[maybe_unused]] const int pitch = bd_pitch(pl.radius), rows = bd_rows(pl.radius), cols = kTW + 2 * p;
    float *S = lds, *R = REF ? lds + pitch * rows : lds;
    int *offs = reinterpret_cast<int *>(lds + pitch * rows * (REF ? 2 : 1));
    const bool lists_in_lds = TILE && !DENSE && bd_tile_bytes(pl.radius, REF) + (long long)kLists * K * 4 <= kLdsBudget;

    if constexpr (TILE) {
        for (int i = tid; i < rows * cols; i += kThreads) {
            const int ly = i / cols, lx = i - ly * cols;
            const int gy = bd_mirror(y0 - p + ly, h), gx = bd_mirror(x0 - p + lx, w);
            S[ly * pitch + lx] = (float)src[(size_t)gy * sstride + gx];
            if constexpr (REF) R[ly * pitch + lx] = (float)ref[(size_t)gy * rstride + gx];
        }
        if constexpr (!DENSE)
            if (lists_in_lds)
                for (int i = tid; i < kLists * K; i += kThreads) offs[i] = bd_offset(pl.pts[2 * i], pl.pts[2 * i + 1], p, pitch);
        __syncthreads();
    }

    const int lx = 4 * (tid & 15), ly = tid >> 4;
    const int x = x0 + lx, y = y0 + ly;
    if (y >= pl.y1 || x >= w) return;
    const float m = pl.m, wmax = pl.wmax;

    BdAcc acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (TILE) {
            acc[e].cen = S[(ly + p) * pitch + lx + p + e];
            acc[e].cen_ref = R[(ly + p) * pitch + lx + p + e];
        } else {
            const int xe = min(x + e, w - 1);
            acc[e].cen = (float)src[(size_t)y * sstride + xe];
            acc[e].cen_ref = REF ? (float)ref[(size_t)y * rstride + xe] : acc[e].cen;
        }
        acc[e].sum = 0.0f;
        acc[e].sum_w = 0.0f;
    }

    if constexpr (DENSE) {
        for (int dy = 0; dy <= 2 * p; ++dy) {
            // column j of this row is the sample at x - p + j; tap dx of output e is column dx + e
            const float *rowS = S + (ly + dy) * pitch + lx, *rowR = R + (ly + dy) * pitch + lx;
            const T *gS = src, *gR = ref;
            if constexpr (!TILE) {
                const int gy = bd_mirror(y - p + dy, h);
                gS = src + (size_t)gy * sstride;
                if constexpr (REF) gR = ref + (size_t)gy * rstride;
            }
            auto load = [&](int j, float &v, float &vr) {
                if constexpr (TILE) {
                    v = rowS[j];
                    vr = REF ? rowR[j] : v;
                } else {
                    const int gx = bd_mirror(x - p + j, w);
                    v = (float)gS[gx];
                    vr = REF ? (float)gR[gx] : v;
                }
            };
            float a0, a1, a2, a3, r0, r1, r2, r3;
            load(0, a0, r0);
            load(1, a1, r1);
            load(2, a2, r2);
            for (int dx = 0; dx <= 2 * p; ++dx) {
                load(dx + 3, a3, r3);
                bd_tap(acc[0], a0, r0, m, wmax);
                bd_tap(acc[1], a1, r1, m, wmax);
                bd_tap(acc[2], a2, r2, m, wmax);
                bd_tap(acc[3], a3, r3, m, wmax);
                a0 = a1, a1 = a2, a2 = a3;
                r0 = r1, r1 = r2, r2 = r3;
            }
        }
    } else {
        const int list = (bd_start(y) + (x >> 2)) % kLists;
        const int16_t *pts = pl.pts + (size_t)list * K * 2;
        const float *baseS = S + ly * pitch + lx, *baseR = R + ly * pitch + lx;
        for (int k = 0; k < K; ++k) {
            if constexpr (TILE) {
                const int o = lists_in_lds ? offs[list * K + k] : bd_offset(pts[2 * k], pts[2 * k + 1], p, pitch);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = baseS[o + e];
                    bd_tap(acc[e], v, REF ? baseR[o + e] : v, m, wmax);
                }
            } else {
                const int px = pts[2 * k], py = pts[2 * k + 1];
                const int gy = bd_mirror(y + py, h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int gx = bd_mirror(x + e + px, w);
                    const float v = (float)src[(size_t)gy * sstride + gx];
                    bd_tap(acc[e], v, REF ? (float)ref[(size_t)gy * rstride + gx] : v, m, wmax);
                }
            }
        }
    }

    T *dp = static_cast<T *>(pl.dst) + (size_t)y * pl.dstride + x;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (x + e < w) dp[e] = bd_finish<T>(acc[e], pl.swmin, pl.peak);
}

template <typename T, bool TILE, bool DENSE>
void launch_ref(bool with_ref, int blocks, size_t lds_bytes, hipStream_t stream, const BdParams &t) {
    if (with_ref)
        hipLaunchKernelGGL((bilateral_dither_kernel<T, TILE, DENSE, true>), dim3(blocks), dim3(kThreads), lds_bytes, stream, t);
    else
        hipLaunchKernelGGL((bilateral_dither_kernel<T, TILE, DENSE, false>), dim3(blocks), dim3(kThreads), lds_bytes, stream, t);
}

template <typename T>
void launch(bool tile, bool dense, bool with_ref, int blocks, size_t lds_bytes, hipStream_t stream, const BdParams &t) {
    if (tile)
        dense ? launch_ref<T, true, true>(with_ref, blocks, lds_bytes, stream, t) : launch_ref<T, true, false>(with_ref, blocks, lds_bytes, stream, t);
    else
        dense ? launch_ref<T, false, true>(with_ref, blocks, 0, stream, t) : launch_ref<T, false, false>(with_ref, blocks, 0, stream, t);
}
#endif  // __HIPCC__

}  // namespace

VSZIP_EXPORT int vszip_bilateral_dither(vszip_ctx *ctx, int dtype, int bits, const vszip_plane *planes, const vszip_bilateral_dither_plane *per, int nplanes) {
    if (!ctx) return VSZIP_ERR_ARG;
    if (!planes || !per || nplanes <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: no planes");
    if (dtype != VSZIP_U8 && dtype != VSZIP_U16 && dtype != VSZIP_F32)
        return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: 8..16-bit integer or 32-bit float planes only");
    if ((dtype == VSZIP_U8 && bits != 8) || (dtype == VSZIP_U16 && (bits < 9 || bits > 16)))
        return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: %d bits per sample do not go with the sample type (8 for 8-bit, 9..16 for 16-bit planes)", bits);
    for (int i = 0; i < nplanes; ++i) {
        const vszip_plane &s = planes[i];
        const vszip_bilateral_dither_plane &q = per[i];
        if (!s.src || !s.dst || s.w <= 0 || s.h <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: plane %d: src and dst must not be NULL", i);
        if (s.dst == s.src || s.dst == s.ref) return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: plane %d: dst must not overlap an input", i);
        if (q.radius < 2 || q.radius > 16384) return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: plane %d: radius %d is outside 2..16384", i, q.radius);
        if (s.w < q.radius || s.h < q.radius) return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: picture size must be greater than \"radius\"");
        if (!q.points && q.K != 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: plane %d: a sub-sampled plane (K = %d) needs its point lists", i, q.K);
        if (q.points && (q.K < 3 || q.K > 4096)) return vszip_set_error(ctx, VSZIP_ERR_ARG, "BilateralDither: plane %d: K = %d is outside 3..4096", i, q.K);
        if (!q.points && q.radius > kMaxDenseRadius)
            return vszip_set_error(ctx, VSZIP_ERR_UNSUPPORTED, "BilateralDither: plane %d: the dense window serves radius <= %d (got %d); use the sub-sampled path (subspl = 0 or >= 4)", i,
                                   kMaxDenseRadius, q.radius);
    }
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));

    const int path = ctx->opt.bilateral_dither_path;  // 0 / 1: the tile where it fits (a forced tile that does not fit goes direct), 2: direct
    const float peak = dtype == VSZIP_F32 ? 0.0f : (float)((1u << bits) - 1);
    BdParams prm;
    int n = 0, blocks = 0;
    long long taps = 0;
    size_t lds_bytes = 0;
    bool cur_tile = false, cur_dense = false, cur_ref = false;
    auto flush = [&]() -> int {
        if (n == 0) return VSZIP_OK;
        prm.nplanes = n;
        {
            vszip_probe_scope probe(ctx);
            if (dtype == VSZIP_U8)
                launch<uint8_t>(cur_tile, cur_dense, cur_ref, blocks, lds_bytes, ctx->stream, prm);
            else if (dtype == VSZIP_U16)
                launch<uint16_t>(cur_tile, cur_dense, cur_ref, blocks, lds_bytes, ctx->stream, prm);
            else
                launch<float>(cur_tile, cur_dense, cur_ref, blocks, lds_bytes, ctx->stream, prm);
        }
        VSZIP_HIP_CHECK(ctx, hipGetLastError());
        n = blocks = 0;
        taps = 0;
        lds_bytes = 0;
        return VSZIP_OK;
    };
    for (int i = 0; i < nplanes; ++i) {
        const vszip_plane &s = planes[i];
        const vszip_bilateral_dither_plane &q = per[i];
        const bool dense = q.points == nullptr, with_ref = s.ref != nullptr && s.ref != s.src;
        const long long tile_bytes = bd_tile_bytes(q.radius, with_ref);
        const bool tile = path != 2 && tile_bytes <= kLdsBudget;
        size_t need = 0;
        if (tile) {
            need = (size_t)tile_bytes;
            if (!dense && tile_bytes + (long long)kLists * q.K * 4 <= kLdsBudget) need += (size_t)kLists * q.K * 4;
        }
        if (n > 0 && (tile != cur_tile || dense != cur_dense || with_ref != cur_ref)) {
            const int rc = flush();
            if (rc != VSZIP_OK) return rc;
        }
        cur_tile = tile, cur_dense = dense, cur_ref = with_ref;
        const long long per_sample = dense ? (long long)(2 * q.radius - 1) * (2 * q.radius - 1) : q.K;
        const long long row_taps = per_sample * s.w;
        const int band = (int)std::min<long long>(std::max<long long>(kTapsPerLaunch / row_taps / kTH * kTH, kTH), ((long long)s.h + kTH - 1) / kTH * kTH);
        for (int y0 = 0; y0 < s.h; y0 += band) {
            const int y1 = std::min(y0 + band, s.h);
            const long long t = row_taps * (y1 - y0);
            if (n > 0 && (n == kBdPlanes || taps + t > kTapsPerLaunch)) {
                const int rc = flush();
                if (rc != VSZIP_OK) return rc;
            }
            BdPlane &d = prm.p[n];
            d.src = s.src;
            d.ref = with_ref ? s.ref : s.src;
            d.dst = s.dst;
            d.pts = q.points;
            d.sstride = (int)s.src_stride;
            d.rstride = with_ref ? (int)s.ref_stride : (int)s.src_stride;
            d.dstride = (int)s.dst_stride;
            d.w = s.w;
            d.h = s.h;
            d.y0 = y0;
            d.y1 = y1;
            d.radius = q.radius;
            d.K = q.K;
            d.tiles_x = (s.w + kTW - 1) / kTW;
            d.m = q.m;
            d.wmax = q.wmax;
            d.swmin = q.sum_w_min;
            d.peak = peak;
            d.block0 = blocks;
            blocks += d.tiles_x * ((y1 - y0 + kTH - 1) / kTH);
            taps += t;
            lds_bytes = std::max(lds_bytes, need);
            ++n;
        }
    }
    return flush();
}
