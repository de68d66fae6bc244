// vszip.MosquitoNR on gfx950 (src/filters/mosquito_nr.zig and mosquito_nr_float.zig as called by
// src/vapoursynth/mosquito_nr.zig): direction-aware smoothing of the sample scaled by 16, then one level of the 5/3
// lifting wavelet of the source and of the smoothed plane, whose LL bands are exchanged (or mixed) before the inverse.
// The reference makes nine full-plane passes over eleven scratch planes; an output sample depends on a 9 x 9
// neighbourhood of the source only, so here a workgroup makes all of it for one tile in LDS: every source sample is
// read about once (tile halos aside), every output sample written once, nothing goes through scratch.
//
// Working types. 8-bit samples: 16-bit two's complement that wraps in every operation, as the reference's i16 with +%
// and -% does (the weighted sums of the smoothing and the LL mix are made in 32 bits and narrowed, as there). 9..16-bit
// samples: 32 bits, where nothing can wrap: a sample is below 2^20, a SAD below 2^23, the smoothing's sum below 2^29
// (weights add up to 256), a wavelet coefficient or a reconstructed value below 2^25 (each lifting step at most triples
// a bound). Float samples: IEEE f32 in the reference's operation order (the library is built without contraction).
//
// Tile. Outputs [X0, X0 + TW) x [Y0, Y0 + TH) with X0, Y0 even, so the lifting parity in the tile is the plane's. The
// inverse transform of an odd output needs its even neighbours, whose approximation coefficient needs the details one
// further out: the smoothed plane and the source's wavelet on [X0 - 2, X0 + TW + 2] x [Y0 - 2, Y0 + TH + 2] (inclusive),
// and the smoothing reads two samples around that: a (TW + 9) x (TH + 9) source footprint. Out-of-plane positions are
// never stored or computed: each consumer resolves them by the reference's rule (reflection without repeating the edge
// for the smoothing; sample n - 2 for the prediction of the last odd sample and the neighbouring detail for the update
// of an end sample), and every rule maps a position to one at most two samples away, inside the tile's own footprint.
//
// Steps of a workgroup (a barrier between each): source -> S (scaled, in the working type); smoothing S -> B on the
// halo of 2; then, in place in both, vertical predict (odd rows), vertical update (even rows), horizontal predict on the
// even rows; one step that makes both LL samples in registers, mixes them and applies the inverse horizontal update;
// inverse horizontal predict; inverse vertical update; and the inverse vertical predict fused with the clamp and the
// store. With restore == 0 the smoothing runs on the tile alone and is stored. Planes with strength == 0 are copied.
//
// Paths. Loads and stores of four samples need bases and pitches that are multiples of four samples (16-byte aligned
// planes are); any other plane is served sample by sample, with the same bits. A four-sample load may cover pitch
// padding (inside h x stride), which lands in LDS columns no consumer reads. Only [0, w) x h is written.
//
// Tile shape: 64 x 32 and 32 x 32 were timed (-DVSZIP_MOSQ_TW / _TH; DESIGN.md 3.12, profiles/mosquito_timing.txt).
#include <algorithm>

#include "plane_table.hpp"

#ifndef VSZIP_MOSQ_TW
#define VSZIP_MOSQ_TW 64
#endif
#ifndef VSZIP_MOSQ_TH
#define VSZIP_MOSQ_TH 32
#endif

namespace {

constexpr int kTW = VSZIP_MOSQ_TW, kTH = VSZIP_MOSQ_TH;  // even; kTW a multiple of 4
constexpr int kHalo = 4;                                 // the source footprint begins at (X0 - 4, Y0 - 4)
constexpr int kPitch = kTW + 12;                         // columns X0 - 4 .. X0 + kTW + 7: whole groups of four
constexpr int kRows = kTH + 9;                           // rows Y0 - 4 .. Y0 + kTH + 4
constexpr int kThreads = 256;
static_assert(kTW % 4 == 0 && kTH % 2 == 0, "tile origin parity and four-sample groups");

struct MosqPlane {
    const void *src;
    void *dst;
    int sstride, dstride, w, h;
    int tiles_x;
    short strength, restore;  // 0 .. 32, 0 .. 128
    short radius, chroma;     // 1 | 2; float planes: the clamp is [-0.5, 0.5]
    int block0;
};
struct MosqParams : PlaneTable<MosqPlane> {
    int maxv;  // integer planes: 2^bits - 1
};

#if defined(__HIPCC__)
// arithmetic of the working type
template <typename W>
struct Ops;
template <>
struct Ops<short> {
    typedef int acc;
    static __device__ __forceinline__ short add(short a, short b) { return (short)(unsigned short)((unsigned)a + (unsigned)b); }
    static __device__ __forceinline__ short sub(short a, short b) { return (short)(unsigned short)((unsigned)a - (unsigned)b); }
    static __device__ __forceinline__ short half(short a) { return (short)(a >> 1); }
    static __device__ __forceinline__ short quarter(short a) { return (short)(a >> 2); }
    static __device__ __forceinline__ short absv(short v) { return std::max(v, sub(0, v)); }
};
template <>
struct Ops<int> {
    typedef int acc;
    static __device__ __forceinline__ int add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
    static __device__ __forceinline__ int sub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
    static __device__ __forceinline__ int half(int a) { return a >> 1; }
    static __device__ __forceinline__ int quarter(int a) { return a >> 2; }
    static __device__ __forceinline__ int absv(int v) { return std::max(v, sub(0, v)); }
};
template <>
struct Ops<float> {
    typedef float acc;
    static __device__ __forceinline__ float add(float a, float b) { return a + b; }
    static __device__ __forceinline__ float sub(float a, float b) { return a - b; }
    static __device__ __forceinline__ float half(float a) { return a * 0.5f; }
    static __device__ __forceinline__ float quarter(float a) { return a * 0.25f; }
    static __device__ __forceinline__ float absv(float v) { return __builtin_fabsf(v); }
};

template <typename T>
struct WorkOf { typedef int type; };
template <>
struct WorkOf<uint8_t> { typedef short type; };
template <>
struct WorkOf<float> { typedef float type; };

template <typename T, typename W>
__device__ __forceinline__ W to_work(T v) {
    if constexpr (std::is_same_v<T, float>)
        return v;
    else
        return (W)((int)v << 4);
}

// reflection without repeating the edge sample, for positions at most two outside [0, n), n >= 4
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// The smoothed sample at a position whose 5 x 5 neighbourhood has the LDS offsets ro[dy + 2] + co[dx + 2].
template <typename W, int R>
__device__ __forceinline__ W smooth_at(const W *S, const int (&ro)[5], const int (&co)[5], int strength) {
    typedef Ops<W> O;
    typedef typename O::acc A;
    auto N = [&](int dx, int dy) -> W { return S[ro[dy + 2] + co[dx + 2]]; };
    const W c = N(0, 0);
    auto t1 = [&](W v) -> W { return O::absv(O::sub(v, c)); };
    auto t2 = [&](W a, W b) -> W { return t1(O::half(O::add(a, b))); };
    auto sum4 = [&](W a, W b, W d, W e) -> A { return (((A)a + (A)b) + (A)d) + (A)e; };
    const W m10 = N(-1, 0), p10 = N(1, 0), z0m1 = N(0, -1), z0p1 = N(0, 1);
    const W m1m1 = N(-1, -1), p1p1 = N(1, 1), p1m1 = N(1, -1), m1p1 = N(-1, 1);
    W sad[8];
    A near[8], far[4] = {0, 0, 0, 0};
    // the half-way directions' four near samples are the same for both radii
    near[4] = sum4(m1m1, m10, p10, p1p1);
    near[5] = sum4(m1m1, z0m1, z0p1, p1p1);
    near[6] = sum4(p1m1, z0m1, z0p1, m1p1);
    near[7] = sum4(p1m1, p10, m10, m1p1);
    if constexpr (R == 1) {
        sad[0] = O::add(t1(m10), t1(p10));
        sad[1] = O::add(t1(m1m1), t1(p1p1));
        sad[2] = O::add(t1(z0m1), t1(z0p1));
        sad[3] = O::add(t1(p1m1), t1(m1p1));
        sad[4] = O::add(t2(m10, m1m1), t2(p10, p1p1));
        sad[5] = O::add(t2(m1m1, z0m1), t2(p1p1, z0p1));
        sad[6] = O::add(t2(z0m1, p1m1), t2(z0p1, m1p1));
        sad[7] = O::add(t2(p10, p1m1), t2(m10, m1p1));
        near[0] = (A)m10 + (A)p10;
        near[1] = (A)m1m1 + (A)p1p1;
        near[2] = (A)z0m1 + (A)z0p1;
        near[3] = (A)p1m1 + (A)m1p1;
    } else {
        const W m20 = N(-2, 0), p20 = N(2, 0), z0m2 = N(0, -2), z0p2 = N(0, 2);
        const W m2m2 = N(-2, -2), p2p2 = N(2, 2), p2m2 = N(2, -2), m2p2 = N(-2, 2);
        const W m2m1 = N(-2, -1), p2p1 = N(2, 1), m1m2 = N(-1, -2), p1p2 = N(1, 2);
        const W p1m2 = N(1, -2), m1p2 = N(-1, 2), p2m1 = N(2, -1), m2p1 = N(-2, 1);
        sad[0] = O::add(O::add(O::add(t1(m10), t1(p10)), t1(m20)), t1(p20));
        sad[1] = O::add(O::add(O::add(t1(m1m1), t1(p1p1)), t1(m2m2)), t1(p2p2));
        sad[2] = O::add(O::add(O::add(t1(z0m1), t1(z0p1)), t1(z0m2)), t1(z0p2));
        sad[3] = O::add(O::add(O::add(t1(p1m1), t1(m1p1)), t1(p2m2)), t1(m2p2));
        // floats: the reference's order is ((a + b) + c) + d
        sad[4] = O::add(O::add(O::add(t1(m2m1), t1(p2p1)), t2(m10, m1m1)), t2(p10, p1p1));
        sad[5] = O::add(O::add(O::add(t1(m1m2), t1(p1p2)), t2(m1m1, z0m1)), t2(p1p1, z0p1));
        sad[6] = O::add(O::add(O::add(t1(p1m2), t1(m1p2)), t2(z0m1, p1m1)), t2(z0p1, m1p1));
        sad[7] = O::add(O::add(O::add(t1(p2m1), t1(m2p1)), t2(p1m1, p10)), t2(m1p1, m10));
        near[0] = sum4(m20, m10, p10, p20);
        near[1] = sum4(m2m2, m1m1, p1p1, p2p2);
        near[2] = sum4(z0m2, z0m1, z0p1, z0p2);
        near[3] = sum4(p2m2, p1m1, m1p1, m2p2);
        far[0] = (A)m2m1 + (A)p2p1;
        far[1] = (A)m1m2 + (A)p1p2;
        far[2] = (A)p1m2 + (A)m1p2;
        far[3] = (A)p2m1 + (A)m2p1;
    }
    // the first strictly smallest SAD
    W bv = sad[0];
    A bn = near[0], bf = 0;
    bool hi = false;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const bool lt = sad[k] < bv;
        bv = lt ? sad[k] : bv;
        bn = lt ? near[k] : bn;
        if (k >= 4) {
            bf = lt ? far[k - 4] : bf;
            hi = lt ? true : hi;
        }
    }
    if (bv == (W)0) return c;  // flat
    if constexpr (std::is_same_v<W, float>) {
        const float s = (float)strength;
        const float coef0 = R == 1 ? 64.0f - 2.0f * s : 128.0f - 4.0f * s, coef1 = R == 1 ? 128.0f - 4.0f * s : 256.0f - 8.0f * s;
        const float inv_lo = R == 1 ? 1.0f / 64.0f : 1.0f / 128.0f, inv_hi = R == 1 ? 1.0f / 128.0f : 1.0f / 256.0f;
        if (!hi) return (coef0 * c + s * bn) * inv_lo;
        if constexpr (R == 1)
            return (coef1 * c + s * bn) * inv_hi;
        else
            return (coef1 * c + (2.0f * s) * bf + s * bn) * inv_hi;
    } else {
        const int s = strength, sh = R == 1 ? 6 : 7;
        const int coef0 = R == 1 ? 64 - 2 * s : 128 - 4 * s, coef1 = 2 * coef0;
        if (!hi) return (W)((coef0 * (int)c + s * bn + (1 << (sh - 1))) >> sh);
        return (W)((coef1 * (int)c + 2 * s * bf + s * bn + (1 << sh)) >> (sh + 1));  // (bf = 0 with radius 1)
    }
}

// where a tile lies in its plane; positions are plane coordinates, LDS offsets come from at()
struct Tile {
    int x0, y0, w, h;
    __device__ __forceinline__ int at(int x, int y) const { return (y - (y0 - kHalo)) * kPitch + (x - (x0 - kHalo)); }
};

// the lifting rules' neighbours of position p of a line of n samples
__device__ __forceinline__ int pred_right(int p, int n) { return p + 1 < n ? p + 1 : p - 1; }  // p odd: sample p + 1, or n - 2
__device__ __forceinline__ int upd_left(int p) { return p >= 1 ? p - 1 : 1; }                   // p even: the detail before, or the first
__device__ __forceinline__ int upd_right(int p, int n) { return p + 1 < n ? p + 1 : p - 1; }    // ... the detail after, or the last

template <typename T>
__device__ __forceinline__ void copy_tile(const MosqPlane &pl, const Tile &t, bool vec) {
    typedef T V4 __attribute__((ext_vector_type(4)));
    const T *src = static_cast<const T *>(pl.src);
    T *dst = static_cast<T *>(pl.dst);
    for (int i = threadIdx.x; i < kTH * (kTW / 4); i += kThreads) {
        const int y = t.y0 + i / (kTW / 4), x = t.x0 + 4 * (i % (kTW / 4));
        if (y >= t.h || x >= t.w) continue;
        const T *s = src + (size_t)y * pl.sstride + x;
        T *d = dst + (size_t)y * pl.dstride + x;
        if (vec && x + 4 <= t.w) {
            *reinterpret_cast<V4 *>(d) = *reinterpret_cast<const V4 *>(s);
        } else {
            for (int k = 0; k < 4 && x + k < t.w; ++k) d[k] = s[k];
        }
    }
}

template <typename T, typename W, int R>
__device__ __forceinline__ void smooth_tile(const W *S, W *B, const Tile &t, int m, int strength) {
    // positions [x0 - m, x0 + kTW + m] x [y0 - m, y0 + kTH + m] of the plane (m = 2), or the tile alone (m = 0)
    const int cols = kTW + (m ? 2 * m + 1 : 0), rows = kTH + (m ? 2 * m + 1 : 0);
    for (int i = threadIdx.x; i < rows * cols; i += kThreads) {
        const int y = t.y0 - m + i / cols, x = t.x0 - m + i % cols;
        if (x < 0 || y < 0 || x >= t.w || y >= t.h) continue;
        int ro[5], co[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            ro[k] = (reflect(y + k - 2, t.h) - (t.y0 - kHalo)) * kPitch;
            co[k] = reflect(x + k - 2, t.w) - (t.x0 - kHalo);
        }
        B[t.at(x, y)] = smooth_at<W, R>(S, ro, co, strength);
    }
}

template <typename T>
__device__ __forceinline__ void mosquito_tile(const MosqPlane &pl, const MosqParams &prm, const Tile &t) {
    typedef typename WorkOf<T>::type W;
    typedef Ops<W> O;
    typedef T V4 __attribute__((ext_vector_type(4)));
    __shared__ W S[kRows * kPitch];
    __shared__ W B[kRows * kPitch];
    const T *src = static_cast<const T *>(pl.src);
    T *dst = static_cast<T *>(pl.dst);
    const int w = t.w, h = t.h, tid = threadIdx.x;
    const bool svec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)((size_t)pl.sstride * sizeof(T))) & (4 * sizeof(T) - 1)) == 0;
    const bool dvec = ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)((size_t)pl.dstride * sizeof(T))) & (4 * sizeof(T) - 1)) == 0;
    const bool wavelet = pl.restore != 0;

    // ---- the source footprint, scaled, in the working type: groups of four samples from x0 - 4 ----
    for (int i = tid; i < kRows * (kPitch / 4); i += kThreads) {
        const int ly = i / (kPitch / 4), lx = 4 * (i % (kPitch / 4));
        const int y = t.y0 - kHalo + ly, x = t.x0 - kHalo + lx;
        if (y < 0 || y >= h || x < 0 || x >= w) continue;  // (x < 0: the whole group, x0 being a multiple of 4)
        const T *s = src + (size_t)y * pl.sstride + x;
        W *o = S + ly * kPitch + lx;
        if (svec) {  // may cover pitch padding: columns at and beyond w of S are not read
            const V4 v = *reinterpret_cast<const V4 *>(s);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = to_work<T, W>(v[k]);
        } else {
            for (int k = 0; k < 4 && x + k < w; ++k) o[k] = to_work<T, W>(s[k]);
        }
    }
    __syncthreads();

    // ---- smoothing ----
    const int m = wavelet ? 2 : 0;
    if (pl.radius == 1)
        smooth_tile<T, W, 1>(S, B, t, m, pl.strength);
    else
        smooth_tile<T, W, 2>(S, B, t, m, pl.strength);
    __syncthreads();

    if (wavelet) {
        constexpr int kCols = kTW + 5;           // columns x0 - 2 .. x0 + kTW + 2
        constexpr int kOdd = kTH / 2 + 2;        // odd rows y0 - 1 .. y0 + kTH + 1
        constexpr int kEven = kTH / 2 + 1;       // even rows y0 .. y0 + kTH
        constexpr int kOddCols = kTW / 2 + 2;    // odd columns x0 - 1 .. x0 + kTW + 1
        constexpr int kEvenCols = kTW / 2 + 1;   // even columns x0 .. x0 + kTW
        // vertical predict: odd rows become details
        for (int i = tid; i < kOdd * kCols; i += kThreads) {
            const int y = t.y0 - 1 + 2 * (i / kCols), x = t.x0 - 2 + i % kCols;
            if (y < 0 || y >= h || x < 0 || x >= w) continue;
            const int a = t.at(x, y), u = t.at(x, y - 1), d = t.at(x, pred_right(y, h));
            B[a] = O::sub(B[a], O::half(O::add(B[u], B[d])));
            S[a] = O::sub(S[a], O::half(O::add(S[u], S[d])));
        }
        __syncthreads();
        // vertical update: even rows become the vertical approximation
        for (int i = tid; i < kEven * kCols; i += kThreads) {
            const int y = t.y0 + 2 * (i / kCols), x = t.x0 - 2 + i % kCols;
            if (y >= h || x < 0 || x >= w) continue;
            const int a = t.at(x, y), u = t.at(x, upd_left(y)), d = t.at(x, upd_right(y, h));
            B[a] = O::add(B[a], O::quarter(O::add(B[u], B[d])));
            S[a] = O::add(S[a], O::quarter(O::add(S[u], S[d])));
        }
        __syncthreads();
        // horizontal predict on the even rows
        for (int i = tid; i < kEven * kOddCols; i += kThreads) {
            const int y = t.y0 + 2 * (i / kOddCols), x = t.x0 - 1 + 2 * (i % kOddCols);
            if (y >= h || x < 0 || x >= w) continue;
            const int a = t.at(x, y), l = t.at(x - 1, y), r = t.at(pred_right(x, w), y);
            B[a] = O::sub(B[a], O::half(O::add(B[l], B[r])));
            S[a] = O::sub(S[a], O::half(O::add(S[l], S[r])));
        }
        __syncthreads();
        // both LL samples, their mix, and the inverse horizontal update with the smoothed plane's details
        for (int i = tid; i < kEven * kEvenCols; i += kThreads) {
            const int y = t.y0 + 2 * (i / kEvenCols), x = t.x0 + 2 * (i % kEvenCols);
            if (y >= h || x >= w) continue;
            const int a = t.at(x, y), l = t.at(upd_left(x), y), r = t.at(upd_right(x, w), y);
            const W qb = O::quarter(O::add(B[l], B[r]));
            const W llb = O::add(B[a], qb), llo = O::add(S[a], O::quarter(O::add(S[l], S[r])));
            W ll = llo;
            if (pl.restore != 128) {
                if constexpr (std::is_same_v<W, float>) {
                    const float wo = (float)pl.restore / 128.0f, wb = 1.0f - wo;
                    ll = wo * llo + wb * llb;
                } else {
                    ll = (W)((pl.restore * (int)llo + (128 - pl.restore) * (int)llb + 64) >> 7);
                }
            }
            B[a] = O::sub(ll, qb);
        }
        __syncthreads();
        // inverse horizontal predict: the odd columns of the tile on the even rows
        for (int i = tid; i < kEven * (kTW / 2); i += kThreads) {
            const int y = t.y0 + 2 * (i / (kTW / 2)), x = t.x0 + 1 + 2 * (i % (kTW / 2));
            if (y >= h || x >= w) continue;
            const int a = t.at(x, y);
            B[a] = O::add(B[a], O::half(O::add(B[t.at(x - 1, y)], B[t.at(pred_right(x, w), y)])));
        }
        __syncthreads();
        // inverse vertical update: the even rows
        for (int i = tid; i < kEven * kTW; i += kThreads) {
            const int y = t.y0 + 2 * (i / kTW), x = t.x0 + i % kTW;
            if (y >= h || x >= w) continue;
            const int a = t.at(x, y);
            B[a] = O::sub(B[a], O::quarter(O::add(B[t.at(x, upd_left(y))], B[t.at(x, upd_right(y, h))])));
        }
        __syncthreads();
    }

    // ---- (inverse vertical predict on the odd rows,) clamp, store: four samples a thread ----
    for (int i = tid; i < kTH * (kTW / 4); i += kThreads) {
        const int y = t.y0 + i / (kTW / 4), x = t.x0 + 4 * (i % (kTW / 4));
        if (y >= h || x >= w) continue;
        const bool odd = wavelet && (y & 1);
        const int a = t.at(x, y), u = t.at(x, y - 1), d = t.at(x, pred_right(y, h));  // (u, d: used on odd rows only)
        V4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            W v = B[a + k];
            if (odd) v = O::add(v, O::half(O::add(B[u + k], B[d + k])));
            if constexpr (std::is_same_v<T, float>) {
                o[k] = fminf(fmaxf(v, pl.chroma ? -0.5f : 0.0f), pl.chroma ? 0.5f : 1.0f);
            } else {
                const int q = (int)O::add(v, (W)8) >> 4;
                o[k] = (T)std::min(std::max(q, 0), prm.maxv);
            }
        }
        T *dp = dst + (size_t)y * pl.dstride + x;
        if (dvec && x + 4 <= w) {
            *reinterpret_cast<V4 *>(dp) = o;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < w) dp[k] = o[k];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void mosquito_kernel(const MosqParams prm) {
    const int b = blockIdx.x;
    const MosqPlane &pl = prm.p[vszip_find_plane(prm, b)];
    const int tile = b - pl.block0, ty = tile / pl.tiles_x, tx = tile - ty * pl.tiles_x;
    const Tile t{tx * kTW, ty * kTH, pl.w, pl.h};
    if (pl.strength == 0) {  // (the whole workgroup: no barrier is skipped by some)
        const uintptr_t bits = reinterpret_cast<uintptr_t>(pl.src) | reinterpret_cast<uintptr_t>(pl.dst) | (uintptr_t)((size_t)pl.sstride * sizeof(T)) |
                               (uintptr_t)((size_t)pl.dstride * sizeof(T));
        copy_tile<T>(pl, t, (bits & (4 * sizeof(T) - 1)) == 0);
        return;
    }
    mosquito_tile<T>(pl, prm, t);
}
#endif  // __HIPCC__

int check_range(vszip_ctx *ctx, const char *key, const int32_t *v, int n, int lo, int hi) {
    // hz.getArray, src/helper.zig:382-400
    for (int i = 0; i < n; ++i) {
        if (v[i] < lo) return vszip_set_error(ctx, VSZIP_ERR_ARG, "MosquitoNR: %s value %d is below minimum %d.", key, (int)v[i], lo);
        if (v[i] > hi) return vszip_set_error(ctx, VSZIP_ERR_ARG, "MosquitoNR: %s value %d is above maximum %d.", key, (int)v[i], hi);
    }
    return VSZIP_OK;
}

}  // namespace

VSZIP_EXPORT int vszip_mosquito_nr(vszip_ctx *ctx, int dtype, int bits_per_sample, const vszip_plane *planes, int nplanes, const int32_t *strength,
                                   const int32_t *restore, const int32_t *radius, const uint8_t *chroma) {
    if (!ctx || !planes || nplanes <= 0) return VSZIP_ERR_ARG;
    // mosquitoNRCreate, src/vapoursynth/mosquito_nr.zig:99-134, in its order
    const bool ok = (dtype == VSZIP_U8 && bits_per_sample == 8) || (dtype == VSZIP_U16 && bits_per_sample >= 9 && bits_per_sample <= 16) || dtype == VSZIP_F32;
    if (!ok) return vszip_set_error(ctx, VSZIP_ERR_ARG, "MosquitoNR: only constant-format 8..16 bit integer or 32 bit float input is supported.");
    if (!strength || !restore || !radius) return vszip_set_error(ctx, VSZIP_ERR_ARG, "MosquitoNR: strength, restore and radius (one value per plane) must not be NULL");
    for (int i = 0; i < nplanes; ++i)
        if (planes[i].w < 4 || planes[i].h < 4) return vszip_set_error(ctx, VSZIP_ERR_ARG, "MosquitoNR: input is too small (need at least 4x4 per processed plane).");
    int rc;
    if ((rc = check_range(ctx, "strength", strength, nplanes, 0, 32)) != VSZIP_OK) return rc;
    if ((rc = check_range(ctx, "restore", restore, nplanes, 0, 128)) != VSZIP_OK) return rc;
    if ((rc = check_range(ctx, "radius", radius, nplanes, 1, 2)) != VSZIP_OK) return rc;
    for (int i = 0; i < nplanes; ++i)
        if (!planes[i].src || !planes[i].dst) return vszip_set_error(ctx, VSZIP_ERR_ARG, "MosquitoNR: plane %d: src and dst must not be NULL", i);
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MosqParams prm;
    prm.maxv = dtype == VSZIP_F32 ? 0 : (1 << bits_per_sample) - 1;
    return vszip_for_each_table(
        ctx, prm, nplanes,
        [&](MosqPlane &d, int i) -> int {
            const vszip_plane &s = planes[i];
            d.src = s.src;
            d.dst = s.dst;
            d.sstride = (int)s.src_stride;
            d.dstride = (int)s.dst_stride;
            d.w = s.w;
            d.h = s.h;
            d.tiles_x = (s.w + kTW - 1) / kTW;
            d.strength = (short)strength[i];
            d.restore = (short)restore[i];
            d.radius = (short)radius[i];
            d.chroma = chroma ? (short)(chroma[i] != 0) : 0;
            return d.tiles_x * ((s.h + kTH - 1) / kTH);
        },
        [&](const MosqParams &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            if (dtype == VSZIP_U8)
                hipLaunchKernelGGL(mosquito_kernel<uint8_t>, dim3(blocks), dim3(kThreads), 0, ctx->stream, t);
            else if (dtype == VSZIP_U16)
                hipLaunchKernelGGL(mosquito_kernel<uint16_t>, dim3(blocks), dim3(kThreads), 0, ctx->stream, t);
            else
                hipLaunchKernelGGL(mosquito_kernel<float>, dim3(blocks), dim3(kThreads), 0, ctx->stream, t);
            return VSZIP_OK;
        });
}
