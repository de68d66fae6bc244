// vszip.CLAHE on gfx950: filter.applyCLAHE (src/filters/clahe.zig:14-282) for a whole table of planes, three launches a plane
// group:
//   clahe_hist_kernel    one workgroup per SLAB (a band of one tile's rows, at most kSlab samples): a private histogram in LDS,
//                        flushed with one global u32 atomic add per non-zero bin into the tile's histogram (scratch, zeroed first);
//                        16-bit: 65 536 bins as packed u16 pairs (128 KiB; a slab of < 65 536 samples cannot carry a half into the
//                        next); 8-bit: 64 copies of the 256 bins, copy = lane, so no two lanes of a wave add to one word
//   clahe_lut_kernel     one workgroup per tile: clip, redistribution, block scan, scaling, into the tile's LUT (sample type, a
//                        region of its own after the group's histograms)
//   clahe_interp_kernel  streaming, 16-byte loads and stores: tx1 / tx2 / xa per sample and ty1 / ty2 / ya per row computed in the
//                        kernel, four LUT lookups per sample (8-bit: the LUTs of the band's tile rows in LDS; 16-bit: gathered
//                        from the L2-resident LUTs)
// Bit-exact with the reference: integer counts in any order, then the reference's f32 operations in its order (-ffp-contract=off).
#include <algorithm>

#include "plane_table.hpp"

namespace {

constexpr int kSlab = 65535;        // samples per histogram workgroup: a packed u16 counter never overflows into its neighbour
constexpr int kHistThreads = 1024;
constexpr int kInterpThreads = 256;
constexpr int kLdsLutBytes = 48 * 1024;  // 8-bit interpolation: LUTs of a band's tile rows held in LDS up to this size

struct CPlane {
    const void *src;
    void *dst;
    uint32_t *hist;  // tiles_x * tiles_y histograms of hist_size words
    void *lut;       // tiles_x * tiles_y LUTs of hist_size samples
    int sstride, dstride, w, h;
    int tx, ty, tw, th;
    uint32_t cl;
    float scale, inv_tw, inv_th;
    int srows;    // rows per slab
    int scw;      // columns per slab (== tw unless a tile row alone exceeds kSlab)
    int schunks;  // column chunks per tile row
    int sper;     // slabs per tile
    int hb0, lb0, ib0;  // first block of this plane in each of the three launches
    int lds;      // 8-bit interpolation: LUTs through LDS
};

typedef PlaneTable<CPlane, 96> CParams;  // 96 planes per launch (32 YUV frames)

template <typename T>
struct Hist;

// 16-bit: word v >> 1 holds bins v & ~1 (low half) and v | 1 (high half)
template <>
struct Hist<uint16_t> {
    static constexpr int kWords = 32768;
    static __device__ __forceinline__ void add(uint32_t *h, uint32_t v, uint32_t n, int) {
        __hip_atomic_fetch_add(&h[v >> 1], n << ((v & 1u) << 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    static __device__ __forceinline__ void flush(const uint32_t *h, uint32_t *g) {
        for (int i = threadIdx.x; i < kWords; i += kHistThreads) {
            const uint32_t c = h[i];
            if (c & 0xffffu) __hip_atomic_fetch_add(&g[2 * i], c & 0xffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c >> 16) __hip_atomic_fetch_add(&g[2 * i + 1], c >> 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

// 8-bit: 64 copies, word bin * 64 + lane (every lane of a wave on a bank of its own)
template <>
struct Hist<uint8_t> {
    static constexpr int kWords = 256 * 64;
    static __device__ __forceinline__ void add(uint32_t *h, uint32_t v, uint32_t n, int lane) {
        __hip_atomic_fetch_add(&h[v * 64 + lane], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    static __device__ __forceinline__ void flush(const uint32_t *h, uint32_t *g) {
        if (threadIdx.x < 256) {
            const uint32_t b = threadIdx.x;
            uint32_t s = 0;
#pragma unroll 16
            for (uint32_t k = 0; k < 64; ++k) s += h[b * 64 + ((k + b) & 63u)];  // rotated: the 32 lanes of a group read 32 banks
            if (s) __hip_atomic_fetch_add(&g[b], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

template <typename T>
__global__ __launch_bounds__(kHistThreads) void clahe_hist_kernel(const CParams prm) {
    constexpr int V = 16 / sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(V)));
    __shared__ __attribute__((aligned(16))) uint32_t h[Hist<T>::kWords];
    const int b = blockIdx.x;
    const CPlane &pl = prm.p[vszip_find_plane(prm, b, &CPlane::hb0)];
    const int local = b - pl.hb0;
    const int tile = local / pl.sper, slab = local - tile * pl.sper;
    const int tyi = tile / pl.tx, txi = tile - tyi * pl.tx;
    const int crow = slab / pl.schunks, cch = slab - crow * pl.schunks;
    const int y0 = tyi * pl.th + crow * pl.srows, y1 = min(y0 + pl.srows, (tyi + 1) * pl.th);
    const int x0 = txi * pl.tw + cch * pl.scw, x1 = min(x0 + pl.scw, (txi + 1) * pl.tw);
    const int lane = threadIdx.x & 63;

    for (int i = threadIdx.x; i < Hist<T>::kWords / 4; i += kHistThreads) reinterpret_cast<uint4 *>(h)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();

    const T *src = static_cast<const T *>(pl.src);
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)((size_t)pl.sstride * sizeof(T))) & 15) == 0;
    const int nrows = y1 - y0;
    if (vec) {
        const int v0 = x0 / V, nvr = (x1 + V - 1) / V - v0;
        const int total = nrows * nvr;
        for (int i = threadIdx.x; i < total; i += kHistThreads) {
            const int r = i / nvr, vi = v0 + (i - r * nvr);
            const VecT v = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(src + (size_t)(y0 + r) * pl.sstride) + vi);
            const int ka = max(x0 - vi * V, 0), kb = min(x1 - vi * V, V);  // the samples of this vector inside the slab
            // equal neighbours within the lane are added as one run (flat and natural content: fewer LDS atomics)
            uint32_t run_v = v[0], run_n = 0;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (k >= ka && k < kb) {
                    if ((uint32_t)v[k] != run_v) {
                        if (run_n) Hist<T>::add(h, run_v, run_n, lane);
                        run_v = v[k];
                        run_n = 0;
                    }
                    ++run_n;
                }
            }
            if (run_n) Hist<T>::add(h, run_v, run_n, lane);
        }
    } else {
        const int cw = x1 - x0, total = nrows * cw;
        for (int i = threadIdx.x; i < total; i += kHistThreads) {
            const int r = i / cw, x = x0 + (i - r * cw);
            Hist<T>::add(h, src[(size_t)(y0 + r) * pl.sstride + x], 1u, lane);
        }
    }
    __syncthreads();
    Hist<T>::flush(h, pl.hist + (size_t)tile * (sizeof(T) == 1 ? 256 : 65536));
}

// clip + redistribute + inclusive scan + scale (calcLut :106-155). NT threads, BPT consecutive bins each. The histogram is read twice
// (L2-warm the second time): first for the clipped excess and the thread's sum, then for the LUT; no bins are held in registers.
template <typename T, int NT>
__global__ __launch_bounds__(NT) void clahe_lut_kernel(const CParams prm) {
    constexpr int HS = sizeof(T) == 1 ? 256 : 65536;
    constexpr int BPT = HS / NT;
    constexpr int NW = NT / 64;
    constexpr int Q = BPT % 4 == 0 ? 4 : 1;  // bins per load
    __shared__ uint32_t red[NW];
    __shared__ uint32_t wsum[NW];
    const int b = blockIdx.x;
    const CPlane &pl = prm.p[vszip_find_plane(prm, b, &CPlane::lb0)];
    const int tile = b - pl.lb0;
    const uint32_t *g = pl.hist + (size_t)tile * HS + threadIdx.x * BPT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t cl = pl.cl;
    auto load = [&](int j, uint32_t *c) {
        if constexpr (Q == 4) {
            const uint4 q = reinterpret_cast<const uint4 *>(g)[j];
            c[0] = q.x, c[1] = q.y, c[2] = q.z, c[3] = q.w;
        } else {
            c[0] = g[j];
        }
    };

    uint32_t ex = 0, kept = 0;
#pragma unroll 4
    for (int j = 0; j < BPT / Q; ++j) {
        uint32_t c[Q];
        load(j, c);
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            ex += c[k] > cl ? c[k] - cl : 0u;
            kept += min(c[k], cl);
        }
    }
    ex = wave_reduce_sum(ex);
    if (lane == 0) red[wave] = ex;
    __syncthreads();
    uint32_t clipped = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) clipped += red[k];
    const uint32_t batch = clipped / HS, residual = clipped - batch * HS;
    // the reference's residual loop (:126-132) adds one to bins 0, step, 2 step, ... (residual of them)
    const uint32_t step = residual ? max((uint32_t)HS / residual, 1u) : 1u;
    const uint32_t lo = tid * BPT, m0 = (lo + step - 1) / step, m1 = min((lo + BPT - 1) / step + 1, residual);
    const uint32_t sum = kept + BPT * batch + (m1 > m0 ? m1 - m0 : 0u);
    const uint32_t inc = wave_incl_scan_dpp(sum);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (int k = 0; k < wave; ++k) run += wsum[k];
    const float scale = pl.scale;
    T *lut = reinterpret_cast<T *>(pl.lut) + (size_t)tile * HS + lo;
    auto entry = [&](uint32_t c, uint32_t i) -> uint32_t {
        run += min(c, cl) + batch + ((residual && i % step == 0 && i / step < residual) ? 1u : 0u);
        return (uint32_t)truncf((float)(int32_t)run * scale + 0.5f);  // P is i32 in the reference
    };
    if constexpr (sizeof(T) == 2 && Q == 4) {
#pragma unroll 2
        for (int j = 0; j < BPT / 8; ++j) {
            uint32_t c[8];
            load(2 * j, c);
            load(2 * j + 1, c + 4);
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t e0 = entry(c[2 * k], lo + 8 * j + 2 * k);
                const uint32_t e1 = entry(c[2 * k + 1], lo + 8 * j + 2 * k + 1);
                w[k] = e0 | (e1 << 16);
            }
            reinterpret_cast<uint4 *>(lut)[j] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        for (int j = 0; j < BPT / Q; ++j) {
            uint32_t c[Q];
            load(j, c);
#pragma unroll
            for (int k = 0; k < Q; ++k) lut[j * Q + k] = (T)entry(c[k], lo + j * Q + k);
        }
    }
}

template <typename T>
struct InterpRows {
    static constexpr int R = sizeof(T) == 1 ? 4 : 2;  // rows per workgroup
};

template <typename T>
__device__ __forceinline__ T clahe_blend(float l0, float l1, float l2, float l3, float xa, float ya, float omy) {
    const float omx = 1.0f - xa;
    const float r = (l0 * omx + l1 * xa) * omy + (l2 * omx + l3 * xa) * ya;
    return (T)(uint32_t)truncf(r + 0.5f);
}

template <typename T>
__global__ __launch_bounds__(kInterpThreads) void clahe_interp_kernel(const CParams prm) {
    constexpr int V = 16 / sizeof(T);
    constexpr int R = InterpRows<T>::R;
    constexpr int HS = sizeof(T) == 1 ? 256 : 65536;
    typedef T VecT __attribute__((ext_vector_type(V)));
    __shared__ __attribute__((aligned(16))) uint8_t lds[sizeof(T) == 1 ? kLdsLutBytes : 16];
    const int b = blockIdx.x;
    const CPlane &pl = prm.p[vszip_find_plane(prm, b, &CPlane::ib0)];
    const int y0 = (b - pl.ib0) * R;
    const T *src = static_cast<const T *>(pl.src);
    T *dst = static_cast<T *>(pl.dst);
    const T *luts = static_cast<const T *>(pl.lut);
    const int txn = pl.tx, tyn = pl.ty;
    const float inv_tw = pl.inv_tw, inv_th = pl.inv_th;
    const int ylast = min(y0 + R, pl.h) - 1;

    // tile rows the band reads: ty1 of its first row .. ty2 of its last (both ascend with y)
    auto trow = [&](int y, int &t1, int &t2, float &ya) {
        const float tyf = (float)y * inv_th - 0.5f;
        const int f = (int)floorf(tyf);
        ya = tyf - (float)f;
        t2 = min(f + 1, tyn - 1);
        t1 = min(max(f, 0), tyn - 1);
    };
    int tlo = 0, nt = 0;
    if (sizeof(T) == 1 && pl.lds) {
        int a, bb, c2, d2;
        float u;
        trow(y0, a, bb, u);
        trow(ylast, c2, d2, u);
        tlo = a;
        nt = (d2 - a + 1) * txn;  // whole LUTs of 256 B
    }
    const bool use_lds = sizeof(T) == 1 && nt > 0 && nt * 256 <= kLdsLutBytes;  // uniform across the workgroup
    if (use_lds) {
        const uint4 *gsrc = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(pl.lut) + (size_t)tlo * txn * 256);
        for (int i = threadIdx.x; i < nt * 16; i += kInterpThreads) reinterpret_cast<uint4 *>(lds)[i] = gsrc[i];
        __syncthreads();
    }

    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)((size_t)pl.sstride * sizeof(T)) |
                       (uintptr_t)((size_t)pl.dstride * sizeof(T))) & 15) == 0;
    for (int y = y0; y <= ylast; ++y) {
        int t1, t2;
        float ya;
        trow(y, t1, t2, ya);
        const float omy = 1.0f - ya;
        const T *s = src + (size_t)y * pl.sstride;
        T *d = dst + (size_t)y * pl.dstride;
        // one sample: the reference's interpolate (:185-281)
        auto one = [&](int x, uint32_t v) -> T {
            const float txf = (float)x * inv_tw - 0.5f;
            const int f = (int)floorf(txf);
            const float xa = txf - (float)f;
            const int x2 = min(f + 1, txn - 1), x1 = min(max(f, 0), txn - 1);
            if (use_lds) {
                const uint8_t *L = lds;
                const int r1 = (t1 - tlo) * txn, r2 = (t2 - tlo) * txn;
                return clahe_blend<T>((float)L[(r1 + x1) * 256 + v], (float)L[(r1 + x2) * 256 + v], (float)L[(r2 + x1) * 256 + v],
                                      (float)L[(r2 + x2) * 256 + v], xa, ya, omy);
            }
            const size_t r1 = (size_t)t1 * txn, r2 = (size_t)t2 * txn;
            return clahe_blend<T>((float)luts[(r1 + x1) * HS + v], (float)luts[(r1 + x2) * HS + v], (float)luts[(r2 + x1) * HS + v],
                                  (float)luts[(r2 + x2) * HS + v], xa, ya, omy);
        };
        int x = 0;
        if (vec) {
            const int nv = pl.w / V;
            for (int i = threadIdx.x; i < nv; i += kInterpThreads) {
                const VecT v = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(s) + i);
                VecT o;
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = one(i * V + k, (uint32_t)v[k]);
                __builtin_nontemporal_store(o, reinterpret_cast<VecT *>(d) + i);
            }
            x = nv * V;
        }
        for (int i = x + threadIdx.x; i < pl.w; i += kInterpThreads) d[i] = one(i, (uint32_t)s[i]);
    }
}

template <typename T>
int run(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, uint32_t limit, int tiles_x, int tiles_y) {
    constexpr uint64_t HS = sizeof(T) == 1 ? 256 : 65536;
    constexpr int R = InterpRows<T>::R;
    // the wrapper's create-time checks (clahe.zig(vs):95-112), on every plane of the table: chroma planes included
    for (int i = 0; i < nplanes; ++i) {
        const vszip_plane &s = planes[i];
        if (!s.src || !s.dst || s.w <= 0 || s.h <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "CLAHE: bad plane %d", i);
        if (tiles_x > s.w || tiles_y > s.h)
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "CLAHE: tiles must not exceed the (chroma) plane width/height (plane %d: %dx%d, tiles %dx%d).", i, s.w,
                                   s.h, tiles_x, tiles_y);
        const uint64_t tot = (uint64_t)(s.w / tiles_x) * (uint64_t)(s.h / tiles_y);
        if ((uint64_t)limit * tot / HS > (uint64_t)INT32_MAX)
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "CLAHE: limit too large for this frame size; reduce limit or increase tiles (plane %d).", i);
    }
    // plane groups: histogram storage of a group within the cap (a plane alone may exceed it: planes are never split). Every plane of
    // the table has the same number of tiles, hence the same storage.
    const size_t cap = (size_t)std::max(ctx->opt.clahe_scratch_mib, 1) << 20;
    const size_t hbytes = (size_t)tiles_x * tiles_y * HS * 4, lbytes = (size_t)tiles_x * tiles_y * HS * sizeof(T);
    const int per_group = (int)std::max<size_t>(1, std::min<size_t>(CParams::capacity, cap / (hbytes + lbytes)));
    const int gmax = std::min(per_group, nplanes);
    scratch::Layout lay;  // [histograms of the group][LUTs of the group]
    const scratch::Region<char> hist = lay.take<char>(hbytes * gmax), lut = lay.take<char>(lbytes * gmax);
    char *base;
    int rc = vszip_reserve_scratch(ctx, lay, &base);
    if (rc != VSZIP_OK) return rc;

    for (int done = 0; done < nplanes;) {
        CParams prm;
        int n = 0, hb = 0, lb = 0, ib = 0;
        size_t grp = 0;
        for (; done + n < nplanes && n < per_group; ++n) {
            const vszip_plane &s = planes[done + n];
            CPlane &d = prm.p[n];
            d.src = s.src;
            d.dst = s.dst;
            d.hist = reinterpret_cast<uint32_t *>(hist.in(base) + hbytes * n);
            d.lut = lut.in(base) + lbytes * n;
            grp += hbytes;
            d.sstride = (int)s.src_stride;
            d.dstride = (int)s.dst_stride;
            d.w = s.w;
            d.h = s.h;
            d.tx = tiles_x;
            d.ty = tiles_y;
            d.tw = s.w / tiles_x;
            d.th = s.h / tiles_y;
            const uint64_t tot = (uint64_t)d.tw * d.th;
            d.cl = (uint32_t)std::max<uint64_t>((uint64_t)limit * tot / HS, 1);
            d.scale = (float)(HS - 1) / (float)tot;
            d.inv_tw = 1.0f / (float)d.tw;
            d.inv_th = 1.0f / (float)d.th;
            // slab split: whole tile rows while they fit kSlab samples, else column chunks of a single row
            if (d.tw <= kSlab) {
                d.srows = std::min(kSlab / d.tw, d.th);
                d.scw = d.tw;
                d.schunks = 1;
            } else {
                d.srows = 1;
                d.schunks = (d.tw + kSlab - 1) / kSlab;
                d.scw = (d.tw + d.schunks - 1) / d.schunks;
            }
            d.sper = d.schunks * ((d.th + d.srows - 1) / d.srows);
            d.hb0 = hb;
            d.lb0 = lb;
            d.ib0 = ib;
            hb += tiles_x * tiles_y * d.sper;
            lb += tiles_x * tiles_y;
            ib += (s.h + R - 1) / R;
            // 8-bit: do the LUTs of the tile rows a band of R rows can touch (ceil((R - 1) / th) + 2, one more for rounding) fit the LDS
            // buffer? (the kernel checks the band's actual count again)
            const int band_trows = std::min(tiles_y, (R - 1 + d.th - 1) / d.th + 3);
            d.lds = (size_t)band_trows * tiles_x * 256 <= (size_t)kLdsLutBytes;
        }
        prm.nplanes = n;
        VSZIP_HIP_CHECK(ctx, hipMemsetAsync(hist.in(base), 0, grp, ctx->stream));
        {
            vszip_probe_scope probe(ctx);
            hipLaunchKernelGGL((clahe_hist_kernel<T>), dim3(hb), dim3(kHistThreads), 0, ctx->stream, prm);
            if constexpr (sizeof(T) == 1)
                hipLaunchKernelGGL((clahe_lut_kernel<T, 256>), dim3(lb), dim3(256), 0, ctx->stream, prm);
            else
                hipLaunchKernelGGL((clahe_lut_kernel<T, 1024>), dim3(lb), dim3(1024), 0, ctx->stream, prm);
            hipLaunchKernelGGL((clahe_interp_kernel<T>), dim3(ib), dim3(kInterpThreads), 0, ctx->stream, prm);
        }
        VSZIP_HIP_CHECK(ctx, hipGetLastError());
        done += n;
    }
    return VSZIP_OK;
}

}  // namespace

VSZIP_EXPORT int vszip_clahe(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes, uint32_t limit, int tiles_x, int tiles_y) {
    if (!ctx) return VSZIP_ERR_ARG;
    if (!planes || nplanes <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "CLAHE: no planes");
    if (dtype != VSZIP_U8 && dtype != VSZIP_U16) return vszip_set_error(ctx, VSZIP_ERR_ARG, "CLAHE: only 8 or 16 bit int formats supported.");
    if (tiles_x < 1 || tiles_y < 1) return vszip_set_error(ctx, VSZIP_ERR_ARG, "CLAHE: tiles values must be >= 1.");
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return dtype == VSZIP_U8 ? run<uint8_t>(ctx, planes, nplanes, limit, tiles_x, tiles_y) : run<uint16_t>(ctx, planes, nplanes, limit, tiles_x, tiles_y);
}
