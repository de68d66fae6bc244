// Host check of the arithmetic and the argument checks of vszip_depth_fmt: a stand-alone program, built by tests/test_depth_fmt_host.py with the
// host compiler under AddressSanitizer + UndefinedBehaviorSanitizer together with vapoursynth-zip_amd/csrc/host_params.cpp. It runs the
// functions of csrc/depth_fmt.hpp (the ones the kernels call) over every code value of 8, 9, 10, 12 and 16 bits and over a grid of floats a
// quarter step apart that overshoots the range at both ends, for {limited, full} x {luma, chroma}, and prints a position-weighted checksum of
// the result bits per case; the test compares them with the numpy specification (tests/depth_fmt_ref.py). Then it sweeps
// vszip_depth_fmt_check over its refusals and prints each call's arguments, code and text.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/vszip_hip.h"
#include "depth_fmt.hpp"

namespace df = depth_fmt;

static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

struct Sum {
    uint64_t s = 0, i = 0;
    void add(uint32_t v) { s += (uint64_t)v * (2 * i + 1), ++i; }
};

static void arithmetic(int bits, int full, int chroma) {
    const df::Range r = df::range_of(bits, full != 0, chroma != 0);
    const df::ToFloat t = df::to_float_of(r);
    const float peak = (float)((1u << bits) - 1u);
    Sum to_float, to_int, round_trip;
    for (uint32_t v = 0; v < (1u << bits); ++v) {
        const float f = df::int_to_float((float)v, t.mul, t.add);
        to_float.add(bits_of(f));
        round_trip.add((uint32_t)df::float_to_int_none(f, (float)r.rng, (float)r.off, peak));
    }
    const long n = ((1l << bits) + 16) * 4;
    for (long k = 0; k < n; ++k) {
        const float x = (float)(((double)k * 0.25 - 8.0 - (double)r.off) / (double)r.rng);
        to_int.add((uint32_t)df::float_to_int_none(x, (float)r.rng, (float)r.off, peak));
    }
    const float inf = std::numeric_limits<float>::infinity();
    for (float x : {inf, -inf, 0.0f, -0.0f, 1.0f, -1.0f}) to_int.add((uint32_t)df::float_to_int_none(x, (float)r.rng, (float)r.off, peak));
    printf("arith %d %d %d off %d rng %d mul %08x add %08x to_float %llu to_int %llu round_trip %llu\n", bits, full, chroma, r.off, r.rng, bits_of(t.mul), bits_of(t.add),
           (unsigned long long)to_float.s, (unsigned long long)to_int.s, (unsigned long long)round_trip.s);
}

struct P {
    int has_src, has_dst, w, h;
    long ss, ds;
    int chroma;
};

static void check(int din, int bin, int dout, int bout, int dither, int full, const std::vector<P> &ps) {
    static char mem[16];
    std::vector<vszip_depth_plane> planes;
    for (const P &p : ps) planes.push_back({p.has_src ? mem : nullptr, (ptrdiff_t)p.ss, p.has_dst ? mem : nullptr, (ptrdiff_t)p.ds, p.w, p.h, p.chroma});
    char err[256];
    std::memset(err, 'x', sizeof err);
    const int rc = vszip_depth_fmt_check(din, bin, dout, bout, dither, full, planes.empty() ? nullptr : planes.data(), (int)planes.size(), err, sizeof err);
    const int quiet = vszip_depth_fmt_check(din, bin, dout, bout, dither, full, planes.empty() ? nullptr : planes.data(), (int)planes.size(), nullptr, 0);
    char tiny[8];
    const int cut = vszip_depth_fmt_check(din, bin, dout, bout, dither, full, planes.empty() ? nullptr : planes.data(), (int)planes.size(), tiny, sizeof tiny);
    printf("check %d %d %d %d %d %d planes %d", din, bin, dout, bout, dither, full, (int)ps.size());
    for (const P &p : ps) printf(" %d %d %d %d %ld %ld %d", p.has_src, p.has_dst, p.w, p.h, p.ss, p.ds, p.chroma);
    printf(" -> %d %d %d %d |%s|\n", rc, quiet, cut, (int)(std::strlen(tiny) < sizeof tiny && std::strncmp(tiny, err, std::strlen(tiny)) == 0), err);
}

int main() {
    for (int bits : {8, 9, 10, 12, 16})
        for (int full = 0; full < 2; ++full)
            for (int chroma = 0; chroma < 2; ++chroma) arithmetic(bits, full, chroma);

    const int U8 = VSZIP_U8, U16 = VSZIP_U16, F16 = VSZIP_F16, F32 = VSZIP_F32;
    static_assert(df::kU8 == VSZIP_U8 && df::kU16 == VSZIP_U16 && df::kF16 == VSZIP_F16 && df::kF32 == VSZIP_F32, "depth_fmt.hpp names the header's dtypes");
    const std::vector<P> ok = {{1, 1, 8, 8, 8, 8, 0}}, ok_chroma = {{1, 1, 8, 8, 8, 8, 0}, {1, 1, 4, 4, 4, 4, 1}};
    // served
    for (int din : {U8, U16, F16, F32})
        for (int dout : {U8, U16, F16, F32})
            for (int dither = 0; dither < 2; ++dither)
                for (int full = 0; full < 2; ++full) check(din, df::bits_hi(din), dout, df::bits_hi(dout), dither, full, ok_chroma);
    for (int bits = 7; bits <= 17; ++bits) check(U16, bits, F32, 32, 0, 0, ok), check(F16, 16, U16, bits, 0, 0, ok);
    // refused
    for (int dt : {-1, 4, 5, 100}) check(dt, 8, F32, 32, 0, 0, ok), check(U8, 8, dt, 32, 0, 0, ok), check(dt, 8, dt, 8, 0, 0, ok);
    check(U8, 9, F32, 32, 0, 0, ok), check(U8, 8, F32, 16, 0, 0, ok), check(F16, 32, U8, 8, 0, 0, ok), check(F32, 32, F16, 32, 0, 0, ok), check(F32, 0, U8, 8, 0, 0, ok);
    for (int dither : {-1, 2, 3}) check(F32, 32, U8, 8, dither, 1, ok), check(U8, 8, F32, 32, dither, 1, ok), check(U16, 16, U8, 8, dither, 0, ok);
    check(U8, 8, F32, 32, 1, 0, ok), check(U16, 10, F16, 16, 1, 1, ok), check(F32, 32, F16, 16, 1, 0, ok), check(F16, 16, F32, 32, 1, 1, ok);
    check(F32, 32, U8, 8, 0, 0, {}), check(U8, 8, U8, 8, 0, 0, {});
    check(F32, 32, U8, 8, 0, 0, {{0, 1, 8, 8, 8, 8, 0}}), check(F32, 32, U8, 8, 0, 0, {{1, 1, 8, 8, 8, 8, 0}, {1, 0, 8, 8, 8, 8, 0}});
    for (const P &p : std::vector<P>{{1, 1, 0, 8, 8, 8, 0}, {1, 1, 8, 0, 8, 8, 0}, {1, 1, 8, 8, 7, 8, 0}, {1, 1, 8, 8, 8, 7, 0}, {1, 1, -3, 8, 8, 8, 0}, {1, 1, 8, 8, 1l << 31, 8, 0}})
        check(U8, 8, F32, 32, 0, 0, {ok[0], p}), check(F16, 16, U16, 12, 1, 1, {p});
    check(F32, 32, U8, 8, 1, 0, ok), check(F16, 16, U16, 10, 1, 0, ok), check(F32, 32, U16, 16, 1, 1, ok_chroma), check(F32, 32, U8, 8, 1, 0, ok_chroma);
    check(U16, 16, U8, 8, 1, 1, ok_chroma), check(U8, 8, U16, 16, 0, 1, ok_chroma);
    check(F32, 32, U8, 8, 0, 0, std::vector<P>(3, P{1, 1, 8, 1 << 29, 8, 8, 0}));
    printf("done\n");
    return 0;
}
