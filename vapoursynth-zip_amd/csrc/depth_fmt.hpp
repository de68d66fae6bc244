// The arithmetic of vszip_depth_fmt in plain C++: zimg's integer <-> float steps as oracle/vs_host.py restates them (int_to_float,
// float_to_int), read by the kernels of depth_fmt.hip, by vszip_depth_fmt_check (host_params.cpp) and by tests/depth_fmt_check.cpp.
// IEEE f32; the one multiply-add of either direction is fused (fmaf is written out: the library is built with contraction off).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define DEPTH_FMT_HD __host__ __device__ inline __attribute__((always_inline))  // (host_params.cpp includes no HIP header)
#else
#define DEPTH_FMT_HD inline
#endif

namespace depth_fmt {

// sample types, by the values of enum vszip_dtype
constexpr int kU8 = 0, kU16 = 1, kF16 = 2, kF32 = 3;

inline bool known_dtype(int dtype) { return dtype >= kU8 && dtype <= kF32; }
inline bool is_float(int dtype) { return dtype == kF16 || dtype == kF32; }
inline int sample_bytes(int dtype) { return dtype == kU8 ? 1 : dtype == kF32 ? 4 : 2; }
inline const char *dtype_name(int dtype) { return dtype == kU8 ? "VSZIP_U8" : dtype == kU16 ? "VSZIP_U16" : dtype == kF16 ? "VSZIP_F16" : "VSZIP_F32"; }
// the bits a plane of `dtype` may declare: [lo, hi]
inline int bits_lo(int dtype) { return dtype == kU8 ? 8 : dtype == kU16 ? 9 : dtype == kF16 ? 16 : 32; }
inline int bits_hi(int dtype) { return dtype == kU8 ? 8 : dtype == kF32 ? 32 : 16; }
inline bool bits_fit(int dtype, int bits) { return bits >= bits_lo(dtype) && bits <= bits_hi(dtype); }

// the integer side of a conversion: code value of 0.0 and the code values 1.0 spans
struct Range {
    int off, rng;
};
inline Range range_of(int bits, bool full_range, bool chroma) {
    if (!full_range) return {(chroma ? 128 : 16) << (bits - 8), (chroma ? 224 : 219) << (bits - 8)};
    return {chroma ? 1 << (bits - 1) : 0, (int)((1u << bits) - 1u)};
}

// integer -> float: fmaf(v, mul, add), both constants divided in double and rounded to float once
struct ToFloat {
    float mul, add;
};
inline ToFloat to_float_of(Range r) { return {(float)(1.0 / (double)r.rng), (float)(-(double)r.off / (double)r.rng)}; }
// (with off == 0 add is -0.0f and the result the plain product v * mul, bit for bit: v >= 0, so the product is never -0)
DEPTH_FMT_HD float int_to_float(float v, float mul, float add) { return fmaf(v, mul, add); }

// float -> integer, dither none: half to even, then the clamp (+-Inf clamp; NaN is outside the contract)
DEPTH_FMT_HD float float_to_int_none(float x, float rng, float off, float peak) { return fminf(fmaxf(rintf(fmaf(x, rng, off)), 0.0f), peak); }

}  // namespace depth_fmt
