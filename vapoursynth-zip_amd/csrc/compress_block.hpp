// The arithmetic of vszip.Compress for one 8 x 8 block (src/filters/compress.zig): plain C++ that the kernel (compress.hip) runs on
// a block held in one lane's registers, and that a host program can run as it is (tests/compress_block_check.cpp).
//
// Everything is 32-bit two's complement that wraps (the reference's +% -% *%), made here in unsigned arithmetic; shifts right are
// arithmetic; t16() is the truncation to i16 with which every pass of the reference stores its block. The quantiser's products are
// 64-bit: a coefficient reaches 2^14 and a multiplier 2^18.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VSZIP_HD __host__ __device__ __forceinline__
#else
#define VSZIP_HD inline
#endif

namespace vszip_compress_dsp {

typedef int32_t i32;
typedef uint32_t u32;

VSZIP_HD i32 add(i32 a, i32 b) { return (i32)((u32)a + (u32)b); }
VSZIP_HD i32 sub(i32 a, i32 b) { return (i32)((u32)a - (u32)b); }
VSZIP_HD i32 mul(i32 a, i32 b) { return (i32)((u32)a * (u32)b); }
VSZIP_HD i32 t16(i32 v) { return (i32)(int16_t)(uint16_t)(u32)v; }
template <int N>
VSZIP_HD i32 descale(i32 x) { return add(x, 1 << (N - 1)) >> N; }

// ---- forward DCT: jfdctint "islow", 8-bit (CONST_BITS 13, PASS1_BITS 4); compress.zig:132-200 ----
// One 1-D transform of t[0], t[S], ..., t[7 S], in place, truncated to i16. EVEN_SHIFT < 0: the first pass, whose even outputs
// are scaled up by 2^4 instead of descaled.
template <int S, int OUT_ROUND, int EVEN_SHIFT>
VSZIP_HD void fdct1d(i32 *t) {
    const i32 tmp0 = add(t[0], t[7 * S]), tmp7 = sub(t[0], t[7 * S]), tmp1 = add(t[S], t[6 * S]), tmp6 = sub(t[S], t[6 * S]);
    const i32 tmp2 = add(t[2 * S], t[5 * S]), tmp5 = sub(t[2 * S], t[5 * S]), tmp3 = add(t[3 * S], t[4 * S]), tmp4 = sub(t[3 * S], t[4 * S]);
    const i32 tmp10 = add(tmp0, tmp3), tmp13 = sub(tmp0, tmp3), tmp11 = add(tmp1, tmp2), tmp12 = sub(tmp1, tmp2);
    if constexpr (EVEN_SHIFT < 0) {
        t[0] = t16(mul(add(tmp10, tmp11), 16));
        t[4 * S] = t16(mul(sub(tmp10, tmp11), 16));
    } else {
        t[0] = t16(descale<EVEN_SHIFT>(add(tmp10, tmp11)));
        t[4 * S] = t16(descale<EVEN_SHIFT>(sub(tmp10, tmp11)));
    }
    i32 z1 = mul(add(tmp12, tmp13), 4433);
    t[2 * S] = t16(descale<OUT_ROUND>(add(z1, mul(tmp13, 6270))));
    t[6 * S] = t16(descale<OUT_ROUND>(add(z1, mul(tmp12, -15137))));
    z1 = add(tmp4, tmp7);
    i32 z2 = add(tmp5, tmp6), z3 = add(tmp4, tmp6), z4 = add(tmp5, tmp7);
    const i32 z5 = mul(add(z3, z4), 9633);
    i32 o4 = mul(tmp4, 2446), o5 = mul(tmp5, 16819), o6 = mul(tmp6, 25172), o7 = mul(tmp7, 12299);
    z1 = mul(z1, -7373);
    z2 = mul(z2, -20995);
    z3 = add(mul(z3, -16069), z5);
    z4 = add(mul(z4, -3196), z5);
    o4 = add(o4, add(z1, z3));
    o5 = add(o5, add(z2, z4));
    o6 = add(o6, add(z2, z3));
    o7 = add(o7, add(z1, z4));
    t[7 * S] = t16(descale<OUT_ROUND>(o4));
    t[5 * S] = t16(descale<OUT_ROUND>(o5));
    t[3 * S] = t16(descale<OUT_ROUND>(o6));
    t[S] = t16(descale<OUT_ROUND>(o7));
}

// ---- quantise + dequantise; compress.zig:206-278 ----
// The reference makes level = (bias + prod) >> 21 for prod = coef qmul > 0 and -((bias - prod) >> 21) otherwise, in 64 bits. With
// qmul >= 0 both are sign(coef) ((bias + |coef| qmul) >> 21): one unsigned 64-bit multiply-add of the magnitude, the sign restored
// afterwards, no branch. MPEG-2's deadzone test, (u64)(prod + T1) > 2 T1 with T1 = 2^21 - bias - 1, says |prod| > T1, that is
// bias + |prod| >= 2^21, that is level != 0: a coefficient inside the deadzone gets level 0 from the formula itself, so the test
// is not made a second time. vszip_compress admits 0 <= qmul <= 2^20 and 0 <= deq < 2^15 (vszip_compress_tables stays within
// 2^18 and 5146); the masks below change no admitted value and tell the compiler that a level and a multiplier fit 24-bit
// multiplies.
constexpr int kQmatShift = 21;
constexpr uint64_t kMpegBias = 96 << 13;                    // the intra bias 3/8 in units of 2^-21
constexpr uint64_t kJpegBias = (uint64_t)1 << (kQmatShift - 1);  // round to nearest, symmetric
constexpr i32 kMaxQmul = 1 << 20, kMaxDeq = (1 << 15) - 1;

template <uint64_t BIAS>
VSZIP_HD i32 level_magnitude(i32 coef, i32 qmul) {
    const u32 mag = (u32)(coef < 0 ? -coef : coef);  // <= 2^15: a coefficient is stored as i16
    return (i32)(((BIAS + (uint64_t)mag * (u32)(qmul & (2 * kMaxQmul - 1))) >> kQmatShift) & 0xFFFF);  // (<= 2^14 + 1)
}
// MPEG-2 intra AC (dct_quantize_c, dct_unquantize_mpeg2_intra_c): the magnitude is dequantised, then the sign restored
VSZIP_HD i32 requant_mpeg2(i32 coef, i32 qmul, i32 deq) {
    const i32 mag = mul(level_magnitude<kMpegBias>(coef, qmul), deq & kMaxDeq) >> 4;
    return t16(coef < 0 ? -mag : mag);
}
// MPEG-2 intra DC: dc >= 0 for 8-bit samples (no level shift); the division truncates
VSZIP_HD i32 requant_mpeg2_dc(i32 dc, i32 dc_q, i32 dc_scale) { return t16(mul(add(dc, dc_q >> 1) / dc_q, dc_scale)); }
// JPEG: all 64 coefficients alike
VSZIP_HD i32 requant_jpeg(i32 coef, i32 qmul, i32 deq) {
    const i32 mag = mul(level_magnitude<kJpegBias>(coef, qmul), deq & kMaxDeq);
    return t16(coef < 0 ? -mag : mag);
}

// ---- inverse DCT: simple_idct, 8-bit (ROW_SHIFT 11, COL_SHIFT 20); compress.zig:284-422 ----
constexpr i32 W1 = 22725, W2 = 21407, W3 = 19266, W4 = 16383, W5 = 12873, W6 = 8867, W7 = 4520;

// even part a[0..3] from its start value and c2, c4, c6; odd part e[0..3] from c1, c3, c5, c7. (The reference skips the terms of
// c4..c7 where they are zero; adding them gives the same bits.)
VSZIP_HD void idct_parts(i32 a0, i32 c1, i32 c2, i32 c3, i32 c4, i32 c5, i32 c6, i32 c7, i32 (&a)[4], i32 (&e)[4]) {
    a[0] = add(add(a0, mul(W2, c2)), add(mul(W4, c4), mul(W6, c6)));
    a[1] = sub(add(a0, mul(W6, c2)), add(mul(W4, c4), mul(W2, c6)));
    a[2] = add(sub(sub(a0, mul(W6, c2)), mul(W4, c4)), mul(W2, c6));
    a[3] = sub(add(sub(a0, mul(W2, c2)), mul(W4, c4)), mul(W6, c6));
    e[0] = add(add(mul(W1, c1), mul(W3, c3)), add(mul(W5, c5), mul(W7, c7)));
    e[1] = sub(sub(sub(mul(W3, c1), mul(W7, c3)), mul(W1, c5)), mul(W5, c7));
    e[2] = add(add(sub(mul(W5, c1), mul(W1, c3)), mul(W7, c5)), mul(W3, c7));
    e[3] = sub(add(sub(mul(W7, c1), mul(W5, c3)), mul(W3, c5)), mul(W1, c7));
}

// Row pass in place. A row whose columns 1..7 are all zero becomes t16(8 c0) eight times: NOT what the formula below gives,
// so it stays a select.
VSZIP_HD void idct_row(i32 *r) {
    const bool dc_only = (r[1] | r[2] | r[3] | r[4] | r[5] | r[6] | r[7]) == 0;
    const i32 dc = t16(mul(r[0], 8));
    i32 a[4], e[4];
    idct_parts(add(mul(W4, r[0]), 1 << 10), r[1], r[2], r[3], r[4], r[5], r[6], r[7], a, e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r[k] = dc_only ? dc : t16(add(a[k], e[k]) >> 11);
        r[7 - k] = dc_only ? dc : t16(sub(a[k], e[k]) >> 11);
    }
}

// Column pass of c[0], c[8], ..., c[56] into samples: OFFSET (128 for JPEG) is added before the clamp to 0..255.
template <int OFFSET>
VSZIP_HD void idct_col_put(const i32 *c, uint8_t *out) {
    i32 a[4], e[4];
    idct_parts(mul(W4, add(c[0], 32)), c[8], c[16], c[24], c[32], c[40], c[48], c[56], a, e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const i32 lo = add(add(a[k], e[k]) >> 20, OFFSET), hi = add(sub(a[k], e[k]) >> 20, OFFSET);
        out[8 * k] = (uint8_t)(lo < 0 ? 0 : (lo > 255 ? 255 : lo));
        out[8 * (7 - k)] = (uint8_t)(hi < 0 ? 0 : (hi > 255 ? 255 : hi));
    }
}

// processBlock (compress.zig:432-446) on b[64], raster order, which holds the samples (JPEG: minus 128) and is left holding the
// row pass of the inverse transform; `out` receives the 64 samples. qmul / deq: the 64 multipliers of the plane's table.
template <int CODEC>
VSZIP_HD void process_block(i32 (&b)[64], uint8_t (&out)[64], const i32 *qmul, const i32 *deq, i32 dc_q, i32 dc_scale) {
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct1d<1, 13 - 4, -1>(b + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct1d<8, 13 + 4, 4>(b + c);
    if constexpr (CODEC == 0) {
        b[0] = requant_mpeg2_dc(b[0], dc_q, dc_scale);
#pragma unroll
        for (int i = 1; i < 64; ++i) b[i] = requant_mpeg2(b[i], qmul[i], deq[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 64; ++i) b[i] = requant_jpeg(b[i], qmul[i], deq[i]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) idct_row(b + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) idct_col_put<CODEC == 1 ? 128 : 0>(b + c, out + c);
}

}  // namespace vszip_compress_dsp
