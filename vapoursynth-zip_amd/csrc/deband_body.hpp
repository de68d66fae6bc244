// The workgroup bodies of the Deband kernels (deband.hip), written against a thread index given as an argument, so that the same
// text runs as host code too: a stand-alone program calls them for tid = 0 .. 255, first the staging, then the samples, with the LDS
// tile as a heap array of the same size, under AddressSanitizer / UBSan.
#pragma once
#include <algorithm>
#include <type_traits>

#include "deband_math.hpp"

namespace deband {

constexpr int kTW = 64, kTH = 32, kThreads = 256;
constexpr int kHaloSmall = 16, kHaloLarge = 32;  // LDS: (64 + 2 H) x (32 + 2 H) samples: 12 / 24 KiB of 16-bit, 24 / 48 KiB of float samples
constexpr int kAngleDistance = 20;

struct DebPlane {
    const void *src;
    void *dst;
    const int8_t *off;   // pairs
    const void *grain;   // int16 | f32, or nullptr
    const float *angle;  // mode 7: scratch, pitch w
    int sstride, dstride, ostride, gstride, w, h;
    int tiles_x;
    float thr, thr1, thr2, lo, hi;
    short ssw, ssh;
    int block0;
};

template <typename T>
struct GrainOf { typedef short type; };
template <>
struct GrainOf<float> { typedef float type; };

VSZIP_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// mode 7, first kernel: the normalised gradient angle of every sample of a 64 x 32 tile
template <typename T>
VSZIP_HD void angle_tile(const DebPlane &pl, int tx, int ty, int tid) {
    const T *src = static_cast<const T *>(pl.src);
    float *out = const_cast<float *>(pl.angle);
    const int w = pl.w, h = pl.h;
    for (int i = tid; i < kTW * kTH; i += kThreads) {
        const int y = ty * kTH + i / kTW, x = tx * kTW + i % kTW;
        if (y >= h || x >= w) continue;
        const int xm = std::max(x - kAngleDistance, 0), xp = std::min(x + kAngleDistance, w - 1);
        const int ym = std::max(y - kAngleDistance, 0), yp = std::min(y + kAngleDistance, h - 1);
        const T *r0 = src + (size_t)ym * pl.sstride, *r1 = src + (size_t)y * pl.sstride, *r2 = src + (size_t)yp * pl.sstride;
        out[(size_t)y * w + x] = gradient_angle((float)r0[xm], (float)r0[x], (float)r0[xp], (float)r1[xm], (float)r1[xp], (float)r2[xm], (float)r2[x], (float)r2[xp]);
    }
}

template <int HALO>
struct TileShape {
    static constexpr int kPitch = kTW + 2 * HALO, kRows = kTH + 2 * HALO;
};

// tile path, before the barrier: the tile and its halo, clipped to the plane, into tileS
template <typename T, int HALO>
VSZIP_HD void stage_tile(const DebPlane &pl, int x0, int y0, int tid, T *tileS) {
    typedef T V4 __attribute__((ext_vector_type(4)));
    constexpr int kPitch = TileShape<HALO>::kPitch, kRows = TileShape<HALO>::kRows;
    const T *src = static_cast<const T *>(pl.src);
    const int w = pl.w, h = pl.h, sstride = pl.sstride;
    const bool svec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)((size_t)sstride * sizeof(T))) & (4 * sizeof(T) - 1)) == 0;
    for (int i = tid; i < kRows * (kPitch / 4); i += kThreads) {
        const int ly = i / (kPitch / 4), lx = 4 * (i % (kPitch / 4));
        const int y = y0 - HALO + ly, x = x0 - HALO + lx;
        if (y < 0 || y >= h || x < 0 || x >= w) continue;  // (x < 0: the whole group, x0 - HALO being a multiple of 4)
        const T *s = src + (size_t)y * sstride + x;
        T *o = tileS + ly * kPitch + lx;
        if (svec) {  // may cover pitch padding: LDS columns at and beyond w are not read
            const V4 v = *reinterpret_cast<const V4 *>(s);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = v[k];
        } else {
            for (int k = 0; k < 4 && x + k < w; ++k) o[k] = s[k];
        }
    }
}

// the samples of a tile; HALO == 0: the direct path (tileS is not used)
template <typename T, int MODE, int HALO>
VSZIP_HD void make_tile(const DebPlane &pl, float angle_boost, float max_angle, int blur_first, int x0, int y0, int tid, const T *tileS) {
    typedef typename GrainOf<T>::type G;
    typedef T V4 __attribute__((ext_vector_type(4)));
    typedef G G4 __attribute__((ext_vector_type(4)));
    typedef char C8 __attribute__((ext_vector_type(8)));
    constexpr bool kFloat = std::is_same_v<T, float>;
    constexpr int kPitch = TileShape<HALO>::kPitch;
    const int w = pl.w, h = pl.h;
    const T *src = static_cast<const T *>(pl.src);
    T *dst = static_cast<T *>(pl.dst);
    const G *grain = static_cast<const G *>(pl.grain);
    const int sstride = pl.sstride;

    uintptr_t bits = (reinterpret_cast<uintptr_t>(src) | (uintptr_t)((size_t)sstride * sizeof(T))) & (4 * sizeof(T) - 1);
    bits |= (reinterpret_cast<uintptr_t>(dst) | (uintptr_t)((size_t)pl.dstride * sizeof(T))) & (4 * sizeof(T) - 1);
    bits |= (reinterpret_cast<uintptr_t>(pl.off) | (uintptr_t)((size_t)pl.ostride * 2)) & 7;
    if (grain) bits |= (reinterpret_cast<uintptr_t>(grain) | (uintptr_t)((size_t)pl.gstride * sizeof(G))) & (4 * sizeof(G) - 1);
    const bool vec = bits == 0;

    // what the gathers may touch: the plane (direct), or the staged rectangle clipped to the plane (tile)
    const int gx0 = HALO ? std::max(x0 - HALO, 0) : 0, gx1 = HALO ? std::min(x0 + kTW + HALO, w) - 1 : w - 1;
    const int gy0 = HALO ? std::max(y0 - HALO, 0) : 0, gy1 = HALO ? std::min(y0 + kTH + HALO, h) - 1 : h - 1;
    auto sample = [&](int x, int y) -> T {
        x = clampi(x, gx0, gx1);
        y = clampi(y, gy0, gy1);
        if constexpr (HALO != 0)
            return tileS[(y - (y0 - HALO)) * kPitch + (x - (x0 - HALO))];
        else
            return src[(size_t)y * sstride + x];
    };
    const Consts k{pl.thr, pl.thr1, pl.thr2, angle_boost, blur_first};
    const int ssw = pl.ssw, ssh = pl.ssh;

    for (int i = tid; i < kTH * (kTW / 4); i += kThreads) {
        const int y = y0 + i / (kTW / 4), x = x0 + 4 * (i % (kTW / 4));
        if (y >= h || x >= w) continue;
        const bool full = vec && x + 4 <= w;
        const int n = std::min(4, w - x);
        const int8_t *op = pl.off + 2 * ((size_t)y * pl.ostride + x);
        const G *gp = grain ? grain + (size_t)y * pl.gstride + x : nullptr;
        T *dp = dst + (size_t)y * pl.dstride + x;
        C8 ov;
        V4 cv;
        G4 gv;
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = (G)0;
        if (full) {
            ov = *reinterpret_cast<const C8 *>(op);
            if constexpr (HALO == 0) cv = *reinterpret_cast<const V4 *>(src + (size_t)y * sstride + x);
            if (gp) gv = *reinterpret_cast<const G4 *>(gp);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = e < n;
                ov[2 * e] = in ? (char)op[2 * e] : (char)0;
                ov[2 * e + 1] = in ? (char)op[2 * e + 1] : (char)0;
                if constexpr (HALO == 0) cv[e] = in ? src[(size_t)y * sstride + x + e] : (T)0;
                if (gp && in) gv[e] = gp[e];
            }
        }
        V4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xe = std::min(x + e, w - 1);  // (lanes beyond w repeat the last sample; they are not stored)
            const Pairs p = pairs_of<MODE, kFloat>((int)(signed char)ov[2 * e], (int)(signed char)ov[2 * e + 1], ssw, ssh);
            T c;
            if constexpr (HALO != 0)
                c = sample(xe, y);
            else
                c = cv[e];
            const T r1 = sample(xe + p.dx1, y + p.dy1), r3 = sample(xe - p.dx1, y - p.dy1);
            T r2 = (T)0, r4 = (T)0;
            if constexpr (MODE != 1 && MODE != 3) {
                r2 = sample(xe + p.dx2, y + p.dy2);
                r4 = sample(xe - p.dx2, y - p.dy2);
            }
            bool boost = false;
            if constexpr (MODE == 7) {
                const float *ang = pl.angle;
                auto A = [&](int ax, int ay) -> float { return ang[(size_t)clampi(ay, 0, h - 1) * w + clampi(ax, 0, w - 1)]; };
                const float a0 = A(xe, y);
                // y offsets from the first pair, x offsets from the second as the table holds it (deband_int.zig:263-289)
                const int yo = p.dy1, xo = p.dx2;
                float md = fmax_(fabs_(A(xe, y + yo) - a0), fabs_(A(xe, y - yo) - a0));
                md = fmax_(md, fmax_(fabs_(A(xe + xo, y) - a0), fabs_(A(xe - xo, y) - a0)));
                boost = md <= max_angle;
            }
            if constexpr (kFloat) {
                float v = sample_float<MODE>(c, r1, r2, r3, r4, k, boost);
                v = v + gv[e];
                out[e] = fmax_(pl.lo, fmin_(v, pl.hi));
            } else {
                int v = sample_int<MODE>((int)c, (int)r1, (int)r2, (int)r3, (int)r4, k, boost);
                v += (int)gv[e];
                out[e] = (T)std::max((int)pl.lo, std::min(v, (int)pl.hi));
            }
        }
        if (full) {
            *reinterpret_cast<V4 *>(dp) = out;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) dp[e] = out[e];
        }
    }
}


}  // namespace deband
