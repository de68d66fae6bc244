// vszip.Checkmate on gfx950 (src/filters/checkmate.zig as called by src/vapoursynth/checkmate.zig): 8-bit planes, a
// spatio-temporal dot-crawl reducer that reads rows y - 2, y, y + 2 of frames n - 1, n, n + 1 (columns x - 2, x, x + 2 of
// frame n, clamped) and, with tthr2 > 0, the sample itself of frames n - 2 and n + 2. One pass, one launch per table of
// planes: every input sample is read about once, every output sample written once, nothing goes through scratch.
//
// Work layout. Only rows of one parity meet in an output sample, so a wave owns the rows of ONE parity of a band of
// kBandRows rows of a strip of columns and walks down them: per frame it keeps the sum of the last two rows of its
// parity and the last row itself (the column sum f[y - 2] + 2 f[y] + f[y + 2] is the sum of two such pair sums), 8
// registers per frame where a 5-row window of three frames would take 60. Each step loads one new lane group of each
// input (3 or 5), one step ahead. A lane group is 8 samples (8-byte loads and stores), held as 16-bit lanes of four
// registers: with 16 samples a lane the kernels need 184 / 203 registers (2 waves a SIMD) and were measured 12-19 %
// slower than with 8 (104 / 116 registers, 4 waves), because the arithmetic, not memory, bounds this kernel (DESIGN.md
// 3.11). Column sums, their differences, the weights, the temporal tests and the blend run on packed 16-bit
// instructions, the weighted sum in 32 bits. The horizontal reach is two samples: the first and the last two of a lane
// group take h = 4 c[y] - col(c) from the neighbouring lane (one exchange in each direction per row), and the first and
// the last lane of a wave compute a lane group they do not store (62 of 64 are output), so no wave needs another wave's
// result. Column clamps are made on the data: sample w - 1 of every row of frame n is repeated to the right when it is
// loaded (into the next lane group too, which exists in every wave because lane 63 stores nothing), sample 0 to the left.
//
// Paths. 8-byte loads and stores need 8-byte aligned bases and pitches of every plane of the entry, the neighbours
// included (16-byte aligned planes are); any other entry runs the same code on byte loads and byte stores. Only
// [0, w) x h is written; an 8-byte load of the last lane group may cover pitch padding (inside h x stride), which is
// overwritten (frame n) or only reaches samples that are not stored (the neighbours).
#include <algorithm>

#include "plane_table.hpp"

namespace {

constexpr int kBandRows = 32;   // rows of a band: two waves (one per parity) produce 16 rows each and load 2 more rows of every input
constexpr int kGroupDwords = 2;   // a lane group: the 8 samples a lane holds of a row
constexpr int kGroup = 4 * kGroupDwords;
constexpr int kStripGroups = 62;  // lane groups a wave stores

struct CheckPlane {
    const uint8_t *src, *p1, *n1, *p2, *n2;
    uint8_t *dst;
    int sstride, p1stride, n1stride, p2stride, n2stride, dstride, w, h;
    int strips;  // waves side by side
    int block0;
};
// Capacity. An entry is 88 bytes (six pointers, six pitches); 128 of them are 11 KiB of kernel argument, no more than the
// three-input streaming table (192 x 64 bytes) that every launch of vszip_limit_filter already carries. 128 planes are
// 42 YUV frames: a 64-frame clip is two launches of about a hundred megabytes each.
constexpr int kCheckPlanes = 128;
struct CheckParams : PlaneTable<CheckPlane, kCheckPlanes> {
    int thr_tmax;  // thr + tmax
    int tmax1;     // tmax + 1
    int mult;      // 8192 / tmax
    int tthr2;     // min(tthr2, 256): differences are at most 255
};

#if defined(__HIPCC__)
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef uint32_t group_t __attribute__((ext_vector_type(kGroupDwords)));

struct Row {
    us2 v[2 * kGroupDwords];  // v[2k]: bytes 0 and 2 of dword k, v[2k + 1]: bytes 1 and 3
};
constexpr int kRegs = 2 * kGroupDwords;

__device__ __forceinline__ us2 as_us2(uint32_t x) { return __builtin_bit_cast(us2, x); }
__device__ __forceinline__ uint32_t as_u32(us2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ us2 splat(int v) { return us2{(unsigned short)v, (unsigned short)v}; }
__device__ __forceinline__ us2 sat_sub(us2 a, us2 b) { return __builtin_elementwise_sub_sat(a, b); }
__device__ __forceinline__ us2 vmin(us2 a, us2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ us2 abs_diff(us2 a, us2 b) { return sat_sub(a, b) | sat_sub(b, a); }
__device__ __forceinline__ group_t zero_group() {
    group_t z;
#pragma unroll
    for (int k = 0; k < kGroupDwords; ++k) z[k] = 0;
    return z;
}

__device__ __forceinline__ Row unpack(group_t r) {
    Row o;
#pragma unroll
    for (int k = 0; k < kGroupDwords; ++k) {
        o.v[2 * k] = as_us2(r[k] & 0x00FF00FFu);
        o.v[2 * k + 1] = as_us2((r[k] >> 8) & 0x00FF00FFu);
    }
    return o;
}
__device__ __forceinline__ group_t pack(const us2 *v) {
    group_t o;
#pragma unroll
    for (int k = 0; k < kGroupDwords; ++k) o[k] = as_u32(v[2 * k]) | (as_u32(v[2 * k + 1]) << 8);
    return o;
}

// trunc(n / 10) for -1020 <= n <= 6120 (curr's range), without a divide: 6554 / 65536 = 1 / 10 + 1 / 163840, so
// n * 6554 >> 16 (arithmetic) is floor(n / 10 + n / 163840): floor(n / 10) for 0 <= n < 16384 (the excess stays below
// 0.1, the smallest gap to the next integer), and for -1638 < n < 0 one less than the quotient rounded toward zero
// whether n is a multiple of 10 or not (the deficit is above -0.01) - hence the sign bit is added back.
__device__ __forceinline__ int div10(int n) { return ((n * 6554) >> 16) - (n >> 31); }

// one sample of the spatial form: (cw * (curr / 10) + pw * (c + p1) + nw * (c + n1)) >> 15, saturated. |cw * q| < 2^24 and
// the sum stays below 2^31 (cw + pw + nw = 16384, q <= 612, c + f <= 510).
__device__ __forceinline__ uint32_t blend_one(int curr, uint32_t cw, uint32_t pw, uint32_t nw, uint32_t sp, uint32_t sn) {
    const int s = (int)cw * div10(curr) + (int)(pw * sp) + (int)(nw * sn);
    return (uint32_t)std::min(std::max(s >> 15, 0), 255);
}

// kGroup samples from x0 of a row; samples at and beyond w read as 0 on the byte path
template <bool Vec>
__device__ __forceinline__ group_t load_group(const uint8_t *row, int x0, int w) {
    if constexpr (Vec) {
        return stream_load<true>(reinterpret_cast<const group_t *>(row + x0));  // every sample is read once (band halos aside)
    } else {
        group_t r = zero_group();
#pragma unroll
        for (int k = 0; k < kGroup; ++k)
            if (x0 + k < w) r[k >> 2] |= (uint32_t)row[x0 + k] << (8 * (k & 3));
        return r;
    }
}

// where a lane's group lies in its plane
struct Lane {
    int x0;       // first sample; -kGroup in the first lane of a plane's first strip
    int w;
    bool inside;  // 0 <= x0 < w
    int last;     // w - 1 - x0 where the group holds the plane's last column, and not as its last sample; else -1
};

// a row of frame n with the column clamps made: sample w - 1 repeated to the right, sample 0 to the left
template <bool Vec>
__device__ __forceinline__ group_t load_cur(const uint8_t *row, const Lane &ln) {
    group_t r = zero_group();
    if (ln.inside) {
        r = load_group<Vec>(row, ln.x0, ln.w);
        if (ln.last >= 0) {  // (one lane group of a plane: other waves skip this)
            const int k0 = ln.last >> 2, sh = 8 * (ln.last & 3);
            uint32_t e = 0;
#pragma unroll
            for (int k = 0; k < kGroupDwords; ++k)
                if (k == k0) e = ((r[k] >> sh) & 0xFFu) * 0x01010101u;
            const uint32_t keep = sh == 24 ? 0xFFFFFFFFu : (1u << (sh + 8)) - 1u;  // bytes 0 .. last & 3 of dword k0
#pragma unroll
            for (int k = 0; k < kGroupDwords; ++k) r[k] = k < k0 ? r[k] : (k == k0 ? (r[k] & keep) | (e & ~keep) : e);
        }
    } else if (ln.x0 >= ln.w && ln.x0 < ln.w + 2) {  // columns w and w + 1 begin the next lane group
        const uint32_t e = row[ln.w - 1] * 0x01010101u;
#pragma unroll
        for (int k = 0; k < kGroupDwords; ++k) r[k] = e;
    } else if (ln.x0 == -kGroup) {
        const uint32_t e = row[0] * 0x01010101u;
#pragma unroll
        for (int k = 0; k < kGroupDwords; ++k) r[k] = e;
    }
    return r;
}

// the state of one frame in a wave's walk: the last row of its parity and that row plus the one before
struct Pair {
    Row r, t;
};
__device__ __forceinline__ void start(Pair &s, group_t first, group_t second) {
    const Row a = unpack(first);
    s.r = unpack(second);
#pragma unroll
    for (int i = 0; i < kRegs; ++i) s.t.v[i] = a.v[i] + s.r.v[i];
}
// the next row arrives: -> the column sum around the row that was last (returned in `mid`), which the state then leaves behind
__device__ __forceinline__ Row advance(Pair &s, group_t next, Row &mid) {
    const Row nr = unpack(next);
    Row col;
    mid = s.r;
#pragma unroll
    for (int i = 0; i < kRegs; ++i) {
        const us2 t = s.r.v[i] + nr.v[i];
        col.v[i] = s.t.v[i] + t;
        s.t.v[i] = t;
    }
    s.r = nr;
    return col;
}

template <bool Temporal, bool Vec>
__device__ __forceinline__ void checkmate_band(const CheckPlane &pl, const CheckParams &prm, int ya, int yend, const Lane &ln, bool stores) {
    const int w = pl.w, h = pl.h;
    auto rowc = [&](int y) { return std::min(std::max(y, 0), h - 1); };  // rows 0, 1, h - 2, h - 1 are copies: their windows are loaded (inside the plane) and not used
    auto cur_row = [&](int y) -> group_t { return load_cur<Vec>(pl.src + (size_t)rowc(y) * pl.sstride, ln); };
    auto p1_row = [&](int y) -> group_t { return ln.inside ? load_group<Vec>(pl.p1 + (size_t)rowc(y) * pl.p1stride, ln.x0, w) : zero_group(); };
    auto n1_row = [&](int y) -> group_t { return ln.inside ? load_group<Vec>(pl.n1 + (size_t)rowc(y) * pl.n1stride, ln.x0, w) : zero_group(); };
    auto p2_row = [&](int y) -> group_t { return ln.inside ? load_group<Vec>(pl.p2 + (size_t)y * pl.p2stride, ln.x0, w) : zero_group(); };
    auto n2_row = [&](int y) -> group_t { return ln.inside ? load_group<Vec>(pl.n2 + (size_t)y * pl.n2stride, ln.x0, w) : zero_group(); };

    Pair sc, sp, sn;  // rows y - 2 and y of frames n, n - 1, n + 1
    start(sc, cur_row(ya - 2), cur_row(ya));
    start(sp, p1_row(ya - 2), p1_row(ya));
    start(sn, n1_row(ya - 2), n1_row(ya));
    group_t next_c = cur_row(ya + 2), next_p = p1_row(ya + 2), next_n = n1_row(ya + 2), next_p2 = zero_group(), next_n2 = zero_group();
    if constexpr (Temporal) {
        next_p2 = p2_row(ya);
        next_n2 = n2_row(ya);
    }

    for (int y = ya; y < yend; y += 2) {
        const bool more = y + 2 < yend;
        // the temporal branch needs row y only, which is here already: where it is taken, and its value there
        us2 take[kRegs], avg[kRegs];
        if constexpr (Temporal) {
            const Row p2 = unpack(next_p2), n2 = unpack(next_n2);
            if (more) {
                next_p2 = p2_row(y + 2);
                next_n2 = n2_row(y + 2);
            }
            const us2 t = splat(prm.tthr2);
#pragma unroll
            for (int i = 0; i < kRegs; ++i) {
                const us2 c = sc.r.v[i], p = sp.r.v[i], n = sn.r.v[i];
                // |p1 - n1| < t and |p2 - c| < t and |c - n2| < t: all three of t -sat |d| are not zero
                const us2 all = vmin(vmin(sat_sub(t, abs_diff(p, n)), sat_sub(t, abs_diff(p2.v[i], c))), sat_sub(t, abs_diff(c, n2.v[i])));
                take[i] = splat(0) - vmin(all, splat(1));  // 0xFFFF where the blend is taken
                avg[i] = ((p + c * splat(2) + n) >> 2) & take[i];
            }
        }
        Row c, p, n;  // row y
        const Row colc = advance(sc, next_c, c), colp = advance(sp, next_p, p), coln = advance(sn, next_n, n);
        if (more) {  // the next step's rows, before this step's arithmetic
            next_c = cur_row(y + 4);
            next_p = p1_row(y + 4);
            next_n = n1_row(y + 4);
        }

        // h(x) = -c[y - 2] + 2 c[y] - c[y + 2] = 4 c[y] - col(c), as wrapping 16-bit; curr = h(x - 2) + h(x + 2) + 2 col(c) + 12 c[y]
        us2 hh[kRegs];
#pragma unroll
        for (int i = 0; i < kRegs; ++i) hh[i] = c.v[i] * splat(4) - colc.v[i];
        // samples x0 - 2, x0 - 1 from the lane before and x0 + kGroup, x0 + kGroup + 1 from the lane after (every lane of the wave takes part)
        const us2 from_left = as_us2(__shfl_up(as_u32(us2{hh[kRegs - 2].y, hh[kRegs - 1].y}), 1, 64));
        const us2 from_right = as_us2(__shfl_down(as_u32(us2{hh[0].x, hh[1].x}), 1, 64));

        group_t o;
        if (y < 2 || y >= h - 2) {  // (a whole row: the same for every lane)
            o = pack(c.v);
        } else {
            us2 res[kRegs];
#pragma unroll
            for (int i = 0; i < kRegs; ++i) {
                const us2 left = i >= 2 ? us2{hh[i >= 2 ? i - 2 : 0].y, hh[i].x} : us2{i == 0 ? from_left.x : from_left.y, hh[i].x};
                const us2 right = i < kRegs - 2 ? us2{hh[i].y, hh[i < kRegs - 2 ? i + 2 : 0].x} : us2{hh[i].y, i == kRegs - 2 ? from_right.x : from_right.y};
                const us2 curr = left + right + colc.v[i] * splat(2) + c.v[i] * splat(12);  // -1020 .. 6120 as signed 16-bit
                const us2 tm = splat(prm.thr_tmax), t1 = splat(prm.tmax1), mu = splat(prm.mult), cap = splat(8192);
                const us2 nw = vmin(vmin(sat_sub(tm, abs_diff(coln.v[i], colc.v[i])), t1) * mu, cap);  // (tmax + 1) * (8192 / tmax) <= 16384
                const us2 pw = vmin(vmin(sat_sub(tm, abs_diff(colp.v[i], colc.v[i])), t1) * mu, cap);
                const us2 cw = splat(16384) - nw - pw;
                const us2 cp = c.v[i] + p.v[i], cn = c.v[i] + n.v[i];
                const uint32_t lo = blend_one((short)curr.x, cw.x, pw.x, nw.x, cp.x, cn.x);
                const uint32_t hi = blend_one((short)curr.y, cw.y, pw.y, nw.y, cp.y, cn.y);
                res[i] = as_us2(lo | (hi << 16));
                if constexpr (Temporal) res[i] = avg[i] | (res[i] & ~take[i]);
            }
            o = pack(res);
        }
        if (stores && ln.inside) {
            uint8_t *d = pl.dst + (size_t)y * pl.dstride + ln.x0;
            if (Vec && ln.x0 + kGroup <= w) {
                *reinterpret_cast<group_t *>(d) = o;
            } else {
#pragma unroll
                for (int k = 0; k < kGroup; ++k)
                    if (ln.x0 + k < w) d[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

template <bool Temporal>
__global__ __launch_bounds__(256) void checkmate_kernel(const CheckParams prm) {
    const int b = blockIdx.x;
    const CheckPlane &pl = prm.p[vszip_find_plane(prm, b)];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // rows and row addresses are the same in every lane
    const int unit = (b - pl.block0) * 4 + wave, lane = threadIdx.x & 63;
    // strips side by side, then the other parity, then the next band
    const int half = unit / pl.strips, strip = unit - half * pl.strips;
    const int y0 = (half >> 1) * kBandRows, ya = y0 + (half & 1);
    if (ya >= pl.h) return;  // (no barrier below)
    const int yend = std::min(y0 + kBandRows, pl.h);
    Lane ln;
    ln.x0 = (strip * kStripGroups + lane - 1) * kGroup;
    ln.w = pl.w;
    ln.inside = ln.x0 >= 0 && ln.x0 < pl.w;
    ln.last = ln.inside && pl.w - 1 - ln.x0 < kGroup - 1 ? pl.w - 1 - ln.x0 : -1;
    const bool stores = lane >= 1 && lane <= kStripGroups;
    uintptr_t bits = reinterpret_cast<uintptr_t>(pl.src) | (uintptr_t)pl.sstride | reinterpret_cast<uintptr_t>(pl.dst) | (uintptr_t)pl.dstride |
                     reinterpret_cast<uintptr_t>(pl.p1) | (uintptr_t)pl.p1stride | reinterpret_cast<uintptr_t>(pl.n1) | (uintptr_t)pl.n1stride;
    if (Temporal) bits |= reinterpret_cast<uintptr_t>(pl.p2) | (uintptr_t)pl.p2stride | reinterpret_cast<uintptr_t>(pl.n2) | (uintptr_t)pl.n2stride;
    if ((bits & (kGroup - 1)) == 0)
        checkmate_band<Temporal, true>(pl, prm, ya, yend, ln, stores);
    else
        checkmate_band<Temporal, false>(pl, prm, ya, yend, ln, stores);
}
#endif  // __HIPCC__

}  // namespace

VSZIP_EXPORT int vszip_checkmate(vszip_ctx *ctx, const vszip_plane *planes, const vszip_temporal_nbrs *nbrs, int nplanes, int thr, int tmax, int tthr2) {
    if (!ctx || !planes || !nbrs || nplanes <= 0) return VSZIP_ERR_ARG;
    // checkmateCreate, src/vapoursynth/checkmate.zig:125-153
    if (tmax < 1 || tmax > 255) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Checkmate: tmax value should be in range [1;255].");
    if (tthr2 < 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Checkmate: tthr2 should be non-negative.");
    if (thr < 0 || thr > 255) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Checkmate: thr value should be in range [0;255].");
    const bool temporal = tthr2 > 0;
    for (int i = 0; i < nplanes; ++i)
        if (planes[i].w < 3 || planes[i].h < 5)
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "Checkmate: clip too small; every plane must be at least 3 wide and 5 tall.");
    for (int i = 0; i < nplanes; ++i) {
        if (!planes[i].src || !planes[i].dst) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Checkmate: plane %d: src and dst must not be NULL", i);
        if (!nbrs[i].p1 || !nbrs[i].n1) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Checkmate: plane %d: p1 and n1 (the plane of frames n - 1 and n + 1) must not be NULL", i);
        if (temporal && (!nbrs[i].p2 || !nbrs[i].n2))
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "Checkmate: plane %d: p2 and n2 (the plane of frames n - 2 and n + 2) must not be NULL when tthr2 > 0", i);
    }
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    CheckParams prm;
    prm.thr_tmax = thr + tmax;
    prm.tmax1 = tmax + 1;
    prm.mult = 8192 / tmax;
    prm.tthr2 = std::min(tthr2, 256);
    return vszip_for_each_table(
        ctx, prm, nplanes,
        [&](CheckPlane &d, int i) -> int {
            const vszip_plane &s = planes[i];
            const vszip_temporal_nbrs &t = nbrs[i];
            d.src = static_cast<const uint8_t *>(s.src);
            d.dst = static_cast<uint8_t *>(s.dst);
            d.p1 = static_cast<const uint8_t *>(t.p1);
            d.n1 = static_cast<const uint8_t *>(t.n1);
            d.p2 = temporal ? static_cast<const uint8_t *>(t.p2) : d.src;  // (the spatial kernel has no load from them)
            d.n2 = temporal ? static_cast<const uint8_t *>(t.n2) : d.src;
            d.sstride = (int)s.src_stride;
            d.dstride = (int)s.dst_stride;
            d.p1stride = (int)t.p1_stride;
            d.n1stride = (int)t.n1_stride;
            d.p2stride = temporal ? (int)t.p2_stride : d.sstride;
            d.n2stride = temporal ? (int)t.n2_stride : d.sstride;
            d.w = s.w;
            d.h = s.h;
            d.strips = ((s.w + kGroup - 1) / kGroup + kStripGroups - 1) / kStripGroups;
            const int bands = (s.h + kBandRows - 1) / kBandRows;
            return (d.strips * bands * 2 + 3) / 4;
        },
        [&](const CheckParams &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            hipLaunchKernelGGL(temporal ? checkmate_kernel<true> : checkmate_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}
