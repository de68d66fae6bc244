// The table of planes that travels in a kernel's argument: its layout, the workgroup's lookup of its plane, the host
// loop that fills and launches one table after another, and the streaming (pointwise) kernel built on the three.
#pragma once
#include <type_traits>

#include "common.hpp"

// Planes per launch. The table is kernel-argument bytes, so its size is fixed at compile time; 64 YUV frames are ONE
// launch (since round 4: four 48-plane launches paid four ramps and tails). Tables with another capacity say so in N.
constexpr int kPlanesPerLaunch = 192;

// Plane carries its first workgroup (or work unit) within the launch, ascending over p[]: `int block0` for
// vszip_find_plane(prm, b) and vszip_for_each_table, or members of its own naming looked up through the overload.
template <typename Plane, int N = kPlanesPerLaunch>
struct PlaneTable {
    static constexpr int capacity = N;
    Plane p[N];
    int nplanes;
};

#if defined(__HIPCC__)
// The last plane whose first block is <= b. block0 ascends: eight scalar steps for 192 planes (a linear scan was part
// of every workgroup's fixed cost). `first`: the member that holds the first block, for tables that carry several.
template <typename Table, typename Plane>
__device__ __forceinline__ int vszip_find_plane(const Table &prm, int b, int Plane::*first) {
    int lo = 0, hi = prm.nplanes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b >= prm.p[mid].*first)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
template <typename Table>
__device__ __forceinline__ int vszip_find_plane(const Table &prm, int b) {
    return vszip_find_plane(prm, b, &std::remove_reference_t<decltype(prm.p[0])>::block0);
}
#endif  // __HIPCC__

// The batching loop: planes [0, nplanes) go through `prm` in runs of at most Table::capacity. fill(entry, i) writes
// plane i into its entry and returns its block count (>= 0) or a VSZIP_ERR_* code; launch(prm, blocks, first) enqueues
// the kernel(s) for the filled table, whose entry 0 is plane `first`, and returns VSZIP_OK or an error. The launch-wide
// fields of `prm` are the caller's.
template <typename Table, typename Fill, typename Launch>
int vszip_for_each_table(vszip_ctx *ctx, Table &prm, int nplanes, Fill fill, Launch launch) {
    for (int done = 0; done < nplanes;) {
        int n = 0, blocks = 0;
        for (; done + n < nplanes && n < Table::capacity; ++n) {
            const int nb = fill(prm.p[n], done + n);
            if (nb < 0) return nb;
            prm.p[n].block0 = blocks;
            blocks += nb;
        }
        prm.nplanes = n;
        const int rc = launch(prm, blocks, done);
        if (rc != VSZIP_OK) return rc;
        VSZIP_HIP_CHECK(ctx, hipGetLastError());
        done += n;
    }
    return VSZIP_OK;
}

// ---- streaming kernels: dst = f(in[0], ..., in[NIN - 1]) per sample ---------------------------------------------------
// 16 bytes per lane per access, kRows rows per workgroup, one launch for a whole table of planes; the HBM roofline is
// every byte read once and written once.
//
// Rows per workgroup, measured on 16 4K YUV420P16 frames (tools/ab_stream.sh, round 2): 1 row 0.42 of the HBM
// peak (a workgroup's fixed cost — plane lookup, two half-filled passes over a 480-vector row — dominates),
// 2 rows + non-temporal loads 0.68, 4 rows 0.67. (A pure copy gains from short-lived workgroups in address
// order, profiles/r02_membw.md; with per-workgroup set-up in the way the gain is a few percent.)
// -DVSZIP_STREAM_ROWS=n / -DVSZIP_STREAM_PLAIN_LOADS are how those figures were taken.
#ifndef VSZIP_STREAM_ROWS
#define VSZIP_STREAM_ROWS 2
#endif
constexpr int kStreamRows = VSZIP_STREAM_ROWS;

struct StreamNoExtra {};

template <int NIN, typename Extra = StreamNoExtra>
struct StreamPlane {
    const void *in[NIN];
    void *dst;
    int istride[NIN], dstride, w, h;  // strides in samples
    int block0;
    [[no_unique_address]] Extra x;  // per-plane constants of the filter
};

#if defined(__HIPCC__)
// (8-bit kernels: LLVM's vector-combine pass may split a 16-byte load whose lanes are only ever extracted into byte
// loads, which lose the hint before the backend merges them again — limit_filter.hip is built without that pass,
// build.py FILE_FLAGS, and tests/test_stream_cache_hints.py reads the hints back from the built code)
template <bool NT, typename V>
__device__ __forceinline__ V stream_load(const V *p) {
#ifndef VSZIP_STREAM_PLAIN_LOADS
    if constexpr (NT) return __builtin_nontemporal_load(p);  // every sample is read once
#endif
    return *p;
}

// The body of a streaming kernel of 256 threads over a table of StreamPlane<Op::kInputs, ...>. Op supplies
//   kInputs, kRows          input streams; rows per workgroup
//   kNontemporalLoads       inputs are loaded with the nt hint
//   kLastMayAlias           the last input may be the very rows of the one before it: then it is loaded once
//   f(px, plane.x, prm)     the output sample for the kInputs input samples px[]
template <typename T, typename Op, typename Table>
__device__ __forceinline__ void stream_map_rows(const Table &prm) {
    constexpr int NIN = Op::kInputs, V = 16 / sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(V)));
    const int b = blockIdx.x;
    const auto pl = prm.p[vszip_find_plane(prm, b)];
    const int y0 = (b - pl.block0) * Op::kRows;
    uintptr_t bits = reinterpret_cast<uintptr_t>(pl.dst) | (uintptr_t)((size_t)pl.dstride * sizeof(T));
#pragma unroll
    for (int k = 0; k < NIN; ++k) bits |= reinterpret_cast<uintptr_t>(pl.in[k]) | (uintptr_t)((size_t)pl.istride[k] * sizeof(T));
    const bool vec = (bits & 15) == 0;
    for (int r = 0; r < Op::kRows; ++r) {
        const int y = y0 + r;
        if (y >= pl.h) break;
        const T *s[NIN];
#pragma unroll
        for (int k = 0; k < NIN; ++k) s[k] = static_cast<const T *>(pl.in[k]) + (size_t)y * pl.istride[k];
        T *d = static_cast<T *>(pl.dst) + (size_t)y * pl.dstride;
        int x = 0;
        if (vec) {
            const int nv = pl.w / V;
            for (int i = threadIdx.x; i < nv; i += 256) {
                VecT v[NIN], o;
#pragma unroll
                for (int k = 0; k < NIN; ++k) {
                    const VecT *q = reinterpret_cast<const VecT *>(s[k]) + i;
                    if (Op::kLastMayAlias && k > 0 && k == NIN - 1)
                        v[k] = s[k] == s[k - 1] ? v[k - 1] : stream_load<Op::kNontemporalLoads>(q);
                    else
                        v[k] = stream_load<Op::kNontemporalLoads>(q);
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    T px[NIN];
#pragma unroll
                    for (int k = 0; k < NIN; ++k) px[k] = v[k][e];
                    o[e] = Op::f(px, pl.x, prm);
                }
                __builtin_nontemporal_store(o, reinterpret_cast<VecT *>(d) + i);
            }
            x = nv * V;
        }
        for (int i = x + threadIdx.x; i < pl.w; i += 256) {
            T px[NIN];
#pragma unroll
            for (int k = 0; k < NIN; ++k) px[k] = s[k][i];
            d[i] = Op::f(px, pl.x, prm);
        }
    }
}

// Host side: fill(entry, i) sets plane i's pointers, strides, size and constants (VSZIP_OK or an error); the block
// count follows from the plane's height.
template <typename Op, typename Table, typename Fill>
int stream_map_run(vszip_ctx *ctx, Table &prm, int nplanes, void (*kernel)(const Table), Fill fill) {
    return vszip_for_each_table(
        ctx, prm, nplanes,
        [&](auto &d, int i) {
            const int rc = fill(d, i);
            return rc != VSZIP_OK ? rc : (d.h + Op::kRows - 1) / Op::kRows;
        },
        [&](const Table &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}
#endif  // __HIPCC__
