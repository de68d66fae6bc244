// The per-sample arithmetic of vszip.Deband, shared by the kernels of deband.hip and by host builds of the same text
// (plain C++: a stand-alone program runs it under AddressSanitizer / UBSan against vectors from tests/deband_ref.py).
// Everything here restates the reference operation by operation: processPlane of src/filters/deband_int.zig and
// deband_float.zig, and pow / atan of src/vcl.zig (ports of VCL2's pow_template_f and atan_f) with an fma where the
// reference has @mulAdd and two roundings everywhere else: the library is built with -ffp-contract=off, and mode 7's
// `max_angle_diff <= max_angle` is a discontinuity, so anything short of the same bits is a wrong sample, not 1e-6.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VSZIP_HD __host__ __device__ __forceinline__
#else
#define VSZIP_HD inline
#endif

namespace deband {

VSZIP_HD float fma32(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
VSZIP_HD uint32_t f2u(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}
VSZIP_HD float u2f(uint32_t u) {
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}
VSZIP_HD float fmax_(float a, float b) { return __builtin_fmaxf(a, b); }
VSZIP_HD float fmin_(float a, float b) { return __builtin_fminf(a, b); }
VSZIP_HD float fabs_(float a) { return __builtin_fabsf(a); }
VSZIP_HD float round_(float a) { return __builtin_roundf(a); }  // half away from zero, Zig's @round

// vcl.atan (atan_f)
VSZIP_HD float vcl_atan(float x) {
    const float P3 = 8.05374449538E-2f, P2 = -1.38776856032E-1f, P1 = 1.99777106478E-1f, P0 = -3.33329491539E-1f;
    const float pi_2 = (float)(3.14159265358979323846 * 0.5), pi_4 = (float)(3.14159265358979323846 * 0.25), sqrt2 = 1.41421356237309504880f;
    const float t = fabs_(x);
    const bool notsmal = t >= sqrt2 - 1.0f, notbig = t <= sqrt2 + 1.0f;
    float s = notbig ? pi_4 : pi_2;
    s = notsmal ? s : 0.0f;
    float a = notbig ? t : 0.0f;
    a += notsmal ? -1.0f : 0.0f;
    float b = notbig ? 1.0f : 0.0f;
    b += notsmal ? t : 0.0f;
    const float z = a / b, zz = z * z, z2 = zz * zz;
    float re = fma32(fma32(P3, zz, P2), z2, fma32(P1, zz, P0));
    re = fma32(re, zz * z, z) + s;
    return u2f((f2u(re) & 0x7FFFFFFFu) | (f2u(x) & 0x80000000u));
}

// vcl.pow (pow_template_f) without its overflow / underflow branches, as the reference has it
VSZIP_HD float vcl_pow(float x0, float y) {
    const float ln2f_hi = 0.693359375f, ln2f_lo = -2.12194440e-4f, ln2 = 0.6931471805599453f, log2e = 1.4426950408889634f, sqrt2_half = 0.7071067811865476f;
    const float P0 = 3.3333331174E-1f, P1 = -2.4999993993E-1f, P2 = 2.0000714765E-1f, P3 = -1.6668057665E-1f, P4 = 1.4249322787E-1f, P5 = -1.2420140846E-1f,
                P6 = 1.1676998740E-1f, P7 = -1.1514610310E-1f, P8 = 7.0376836292E-2f;
    const float e2f = 1.0f / 2.0f, e3f = 1.0f / 6.0f, e4f = 1.0f / 24.0f, e5f = 1.0f / 120.0f, e6f = 1.0f / 720.0f, e7f = 1.0f / 5040.0f;
    const float x1 = fabs_(x0);
    const uint32_t bits = f2u(x1);
    float x = u2f((bits & 0x007FFFFFu) | 0x3F000000u);  // fraction_2
    const bool blend = x > sqrt2_half;
    x = blend ? x : x + x;
    x -= 1.0f;
    const float x2 = x * x, x4 = x2 * x2, x8 = x4 * x4;
    float lg1 = fma32(fma32(fma32(P7, x, P6), x2, fma32(P5, x, P4)), x4, fma32(fma32(P3, x, P2), x2, fma32(P1, x, P0) + P8 * x8));  // polynomial_8
    lg1 *= x2 * x;
    float ef = (float)((int32_t)((bits >> 23) & 0xFFu) - 127);  // exponent_f
    ef = blend ? ef + 1.0f : ef;
    const float e1 = round_(ef * y);
    const float yr = fma32(ef, y, -e1);
    const float lg = fma32(0.5f, -x2, x) + lg1;
    const float x2err = fma32(0.5f * x, x, 0.5f * -x2);
    const float lgerr = fma32(0.5f, x2, lg - x) - lg1;
    const float e2 = round_(lg * y * log2e);
    float v = fma32(lg, y, -e2 * ln2f_hi);
    v = fma32(-e2, ln2f_lo, v);
    const float correction = fma32(lgerr + x2err, y, -yr * ln2);
    v -= correction;
    x = v;
    const float e3 = round_(x * log2e);
    x = fma32(-e3, ln2, x);
    const float x2e = x * x, xx4 = x2e * x2e;
    float z = fma32(fma32(e5f, x, e4f), x2e, fma32(fma32(e7f, x, e6f), xx4, fma32(e3f, x, e2f)));  // polynomial_5
    z = z * x2e + x + 1.0f;
    const float ee = e1 + e2 + e3;
    const int32_t ei = (int32_t)round_(ee);
    z = u2f(f2u(z) + ((uint32_t)ei << 23));
    const bool xzero = (f2u(x0) & 0x7F800000u) == 0;
    const float zero_case = y < 0.0f ? u2f(0x7F800000u) : (y == 0.0f ? 1.0f : 0.0f);
    return xzero ? zero_case : z;
}

// calculateGradientAngle from its eight samples (already f32)
VSZIP_HD float gradient_angle(float p00, float p10, float p20, float p01, float p21, float p02, float p12, float p22) {
    const float gx = (p20 + 2.0f * p21 + p22) - (p00 + 2.0f * p01 + p02);
    const float gy = (p00 + 2.0f * p10 + p20) - (p02 + 2.0f * p12 + p22);
    if (fabs_(gx) < (float)(0.01 * 3.0)) return 1.0f;
    return vcl_atan(gy / gx) / 3.14159265358979323846f + 0.5f;
}

struct Consts {
    float thr, thr1, thr2;  // on the plane's scale
    float angle_boost;
    int blur_first;
};

VSZIP_HD float saturate(float x) { return fmax_(0.0f, fmin_(x, 1.0f)); }

// modes 6 and 7: p1, p2 the first pair (refs 1 and 3), p3, p4 the second (refs 2 and 4)
VSZIP_HD float soft_blend(float c, float p1, float p2, float p3, float p4, const Consts &k, bool boost) {
    float t_avg = k.thr, t_max = k.thr1, t_mid = k.thr2;
    if (boost) {
        t_avg = t_avg * k.angle_boost;
        t_max = t_max * k.angle_boost;
        t_mid = t_mid * k.angle_boost;
    }
    const float avg = (p1 + p2 + p3 + p4) * 0.25f;
    const float diff = avg - c;
    const float max_dif = fmax_(fmax_(fabs_(p1 - c), fabs_(p2 - c)), fmax_(fabs_(p3 - c), fabs_(p4 - c)));
    const float two = c * 2.0f;
    const float mid_v = fabs_((p1 + p2) - two), mid_h = fabs_((p3 + p4) - two);
    const float eps = 1e-5f;
    const float comp_avg = saturate(3.0f * (1.0f - fabs_(diff) / fmax_(t_avg, eps)));
    const float comp_max = saturate(3.0f * (1.0f - max_dif / fmax_(t_max, eps)));
    const float comp_mv = saturate(3.0f * (1.0f - mid_v / fmax_(t_mid, eps)));
    const float comp_mh = saturate(3.0f * (1.0f - mid_h / fmax_(t_mid, eps)));
    const float product = comp_avg * comp_max * comp_mv * comp_mh;
    return c + diff * vcl_pow(product, 0.1f);
}

VSZIP_HD int iabs(int v) { return v < 0 ? -v : v; }

// integer samples (16-bit scale, 32-bit arithmetic): the value before grain and clamp
template <int MODE>
VSZIP_HD int sample_int(int c, int r1, int r2, int r3, int r4, const Consts &k, bool boost) {
    const int thr = (int)k.thr;
    if constexpr (MODE == 1 || MODE == 3) {
        const int avg = (r1 + r3 + 1) >> 1;
        const bool orig = k.blur_first ? iabs(avg - c) >= thr : (iabs(r1 - c) >= thr) || (iabs(r3 - c) >= thr);
        return orig ? c : avg;
    } else if constexpr (MODE == 2) {
        int a1 = (r1 + r3 + 1) >> 1;
        const int a2 = (r2 + r4 + 1) >> 1;
        a1 -= a1 > 0 ? 1 : 0;  // avg_4's quirk, "consistent with SSE code"
        const int avg = (a1 + a2 + 1) >> 1;
        const bool orig = k.blur_first ? iabs(avg - c) >= thr : (iabs(r1 - c) >= thr) || (iabs(r2 - c) >= thr) || (iabs(r3 - c) >= thr) || (iabs(r4 - c) >= thr);
        return orig ? c : avg;
    } else if constexpr (MODE == 4) {
        const int av = (r1 + r3 + 1) >> 1, ah = (r2 + r4 + 1) >> 1;
        const bool ov = k.blur_first ? iabs(av - c) >= thr : (iabs(r1 - c) >= thr) || (iabs(r3 - c) >= thr);
        const bool oh = k.blur_first ? iabs(ah - c) >= thr : (iabs(r2 - c) >= thr) || (iabs(r4 - c) >= thr);
        return ((ov ? c : av) + (oh ? c : ah) + 1) >> 1;
    } else if constexpr (MODE == 5) {
        const int thr1 = (int)k.thr1, thr2 = (int)k.thr2;
        const int avg = (r1 + r3 + r2 + r4) >> 2;  // truncated
        const int max_dif = iabs(r1 - c) > iabs(r3 - c) ? iabs(r1 - c) : iabs(r3 - c);
        const int max_dif2 = iabs(r2 - c) > iabs(r4 - c) ? iabs(r2 - c) : iabs(r4 - c);
        const int mx = max_dif > max_dif2 ? max_dif : max_dif2;
        const int m1 = iabs((r1 + r3) - 2 * c), m2 = iabs((r2 + r4) - 2 * c);
        const bool orig = (iabs(avg - c) >= thr) || (mx >= thr1) || (m1 >= thr2) || (m2 >= thr2);
        return orig ? c : avg;
    } else {
        const float bl = soft_blend((float)c, (float)r1, (float)r3, (float)r2, (float)r4, k, boost);
        return (int)__builtin_truncf(bl + 0.5f);
    }
}

// float samples: the value before grain and clamp (sums in the reference's order r1 + r2 + r3 + r4)
template <int MODE>
VSZIP_HD float sample_float(float c, float r1, float r2, float r3, float r4, const Consts &k, bool boost) {
    const float thr = k.thr;
    if constexpr (MODE == 1 || MODE == 3) {
        const float avg = (r1 + r3) * 0.5f;
        const bool orig = k.blur_first ? fabs_(avg - c) >= thr : (fabs_(r1 - c) >= thr) || (fabs_(r3 - c) >= thr);
        return orig ? c : avg;
    } else if constexpr (MODE == 2) {
        const float avg = (r1 + r2 + r3 + r4) * 0.25f;
        const bool orig = k.blur_first ? fabs_(avg - c) >= thr : (fabs_(r1 - c) >= thr) || (fabs_(r2 - c) >= thr) || (fabs_(r3 - c) >= thr) || (fabs_(r4 - c) >= thr);
        return orig ? c : avg;
    } else if constexpr (MODE == 4) {
        const float av = (r1 + r3) * 0.5f, ah = (r2 + r4) * 0.5f;
        const bool ov = k.blur_first ? fabs_(av - c) >= thr : (fabs_(r1 - c) >= thr) || (fabs_(r3 - c) >= thr);
        const bool oh = k.blur_first ? fabs_(ah - c) >= thr : (fabs_(r2 - c) >= thr) || (fabs_(r4 - c) >= thr);
        return ((ov ? c : av) + (oh ? c : ah)) * 0.5f;
    } else if constexpr (MODE == 5) {
        const float avg = (r1 + r2 + r3 + r4) * 0.25f;
        const float mx = fmax_(fmax_(fabs_(r1 - c), fabs_(r2 - c)), fmax_(fabs_(r3 - c), fabs_(r4 - c)));
        const float two = c * 2.0f;
        const float m1 = fabs_((r1 + r3) - two), m2 = fabs_((r2 + r4) - two);
        const bool orig = (fabs_(avg - c) >= thr) || (mx >= k.thr1) || (m1 >= k.thr2) || (m2 >= k.thr2);
        return orig ? c : avg;
    } else {
        return soft_blend(c, r1, r3, r2, r4, k, boost);
    }
}

// The two sample pairs of a table entry: refs 1 / 3 at +-(dx1, dy1), refs 2 / 4 at +-(dx2, dy2). v1 / v2: the table's values,
// shifted by the plane's subsampling. The float path reads the second pair through the absolute value of its flattened
// offset (deband_float.zig:158), which for in-plane offsets is this sign rule.
struct Pairs {
    int dx1, dy1, dx2, dy2;
};
template <int MODE, bool FLOAT>
VSZIP_HD Pairs pairs_of(int v1, int v2, int ssw, int ssh) {
    const int v1w = v1 >> ssw, v1h = v1 >> ssh, v2w = v2 >> ssw, v2h = v2 >> ssh;
    if constexpr (MODE == 1) return Pairs{0, v1h, 0, 0};
    if constexpr (MODE == 3) return Pairs{v1w, 0, 0, 0};
    if constexpr (MODE == 2) {
        const bool neg = FLOAT && (v1h > 0 || (v1h == 0 && v2w < 0));
        return Pairs{v1w, v2h, neg ? -v2w : v2w, neg ? v1h : -v1h};
    }
    return Pairs{0, v1h, FLOAT ? iabs(v1w) : v1w, 0};
}

}  // namespace deband
