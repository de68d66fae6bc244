// Device-free entry points of include/vszip_hip.h — plain C++ (no HIP header), compiled into libvszip_hip.so by
// hipcc and, unchanged, into the sanitizer stub of tests/sanitize (g++ -fsanitize=address,undefined), so that the
// plugin's create-time paths run the real parameter derivation under ASan/UBSan without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/vszip_hip.h"
#include "depth_fmt.hpp"

#define VSZIP_EXPORT extern "C" __attribute__((visibility("default")))

// bilateralCreate's per-plane derivation, src/vapoursynth/bilateral.zig:104-199 (host only).
VSZIP_EXPORT int vszip_bilateral_derive(const double *sigmaS_in, int n_sigmaS, const double *sigmaR, const int *algorithm_in, const int *pbficnum_in,
                                        int is_yuv, int subsampling_w, int subsampling_h, const int *planes_in, vszip_bilateral_cfg *out) {
    if (!sigmaR || !algorithm_in || !pbficnum_in || !planes_in || !out || n_sigmaS < 0 || n_sigmaS > 3) return VSZIP_ERR_ARG;
    double sS[3];
    for (int i = 0; i < 3; ++i) {
        if (i < n_sigmaS)
            sS[i] = sigmaS_in[i];
        else if (i == 0)
            sS[0] = 3;
        else if (i == 1 && is_yuv && subsampling_h != 0 && subsampling_w != 0)
            sS[1] = sS[0] / std::sqrt((double)((1u << subsampling_h) * (1u << subsampling_w)));
        else
            sS[i] = sS[i - 1];
        if (sS[i] < 0) return VSZIP_ERR_ARG;  // "Invalid \"sigmaS\" assigned, must be non-negative float number"
    }
    for (int i = 0; i < 3; ++i) {
        vszip_bilateral_cfg &c = out[i];
        c.sigmaS = sS[i];
        c.sigmaR = sigmaR[i];
        c.process = planes_in[i] && !(sS[i] == 0 || sigmaR[i] == 0);
        c.algorithm = algorithm_in[i];
        c.pbficnum = pbficnum_in[i];
        c.radius = c.step = c.samples = 0;
        c.gs_lut = c.gr_lut = nullptr;
    }
    for (int i = 0; i < 3; ++i)
        if (out[i].pbficnum == 1) return VSZIP_ERR_ARG;  // "must be integer ranges in [0,256] except 1"
    for (int i = 0; i < 3; ++i) {
        vszip_bilateral_cfg &c = out[i];
        if (c.process && c.pbficnum == 0) {
            if (c.sigmaR >= 0.08)
                c.pbficnum = 4;
            else if (c.sigmaR >= 0.015)
                c.pbficnum = std::min(16, (int)std::trunc(4 * 0.08 / c.sigmaR + 0.5));
            else
                c.pbficnum = std::min(32, (int)std::trunc(16 * 0.015 / c.sigmaR + 0.5));
            if (i > 0 && is_yuv && (c.pbficnum % 2 == 0) && c.pbficnum < 256) c.pbficnum += 1;
        }
    }
    for (int i = 0; i < 3; ++i) {
        vszip_bilateral_cfg &c = out[i];
        if (!c.process) continue;
        const int orad = std::max((int)std::trunc(c.sigmaS * 2 + 0.5), 1);
        c.step = orad < 4 ? 1 : (orad < 8 ? 2 : 3);
        c.samples = 1;
        c.radius = 1 + (c.samples - 1) * c.step;
        while (orad * 2 > c.radius * 3) {
            c.samples += 1;
            c.radius = 1 + (c.samples - 1) * c.step;
            if (c.radius >= orad && c.samples > 2) {
                c.samples -= 1;
                c.radius = 1 + (c.samples - 1) * c.step;
                break;
            }
        }
        if (c.algorithm <= 0)
            c.algorithm = (c.step == 1) ? 2 : ((c.sigmaR < 0.08 && c.samples < 5) ? 2 : ((4 * c.samples * c.samples <= 15 * c.pbficnum) ? 2 : 1));
    }
    return VSZIP_OK;
}

// getFrameXPSNR :370-374 on sqrt(f64(wsse)) (src/vapoursynth/xpsnr.zig:84-86). Host only.
VSZIP_EXPORT double vszip_xpsnr_value(uint64_t wsse, uint64_t width, uint64_t height, int depth) {
    const double sq = std::sqrt((double)wsse);
    if (sq < 1) return INFINITY;
    uint64_t maxerr = ((uint64_t)1 << depth) - 1;
    maxerr *= maxerr;
    return 10.0 * std::log10((double)(width * height * maxerr) / (sq * sq));
}

// getAvgXPSNR :359-368: the per-clip average printed by xpsnrFree. Host only.
VSZIP_EXPORT double vszip_xpsnr_average(double sum_wdist, double sum_xpsnr, uint64_t width, uint64_t height, int depth, uint64_t num_frames) {
    const double nf = (double)num_frames;
    uint64_t maxerr = ((uint64_t)1 << depth) - 1;
    maxerr *= maxerr;
    if (sum_wdist >= nf) {
        const double avg = sum_wdist / nf;
        return 10.0 * std::log10((double)(width * height * maxerr) / (avg * avg));
    }
    return sum_xpsnr / nf;
}

// ---------------------------------------------------------------------------------------------------------
// zimg's resampling table for one axis (round 3: the YUV colour pre-stage of SSIMULACRA2) — what
// `resize.Bicubic(format=RGBS)` in hz.toRGBS (src/helper.zig:225-243) uses to bring a subsampled chroma plane to
// 4:4:4. zimg is third-party and not in the reference tree; this restates its published filter construction
// (oracle/vs_host.py::zimg_filter is the twin the tests compare with, itself pinned by the reference's goldens):
// per output sample the window `pos = (i + 0.5) / scale + shift`, `filter_size = ceil(2 * support)` taps starting at
// `floor(pos - filter_size / 2 + 0.5)`, weights normalised, taps outside the line reflected about the edge (edge
// sample repeated) and ADDED to the sample they land on, rows trimmed to their non-zero span and aligned to the common
// width. Upscaling only (scale >= 1, support 2): at most 4 taps. coef4[4 * i + k] multiplies sample left[i] + k; the
// caller clamps left[i] + k to src_dim - 1 for lines shorter than 4 (those coefficients are 0).
// ---------------------------------------------------------------------------------------------------------
namespace {
double bicubic_weight(double x, double b, double c) {
    x = std::fabs(x);
    const double p0 = (6.0 - 2.0 * b) / 6.0, p2 = (-18.0 + 12.0 * b + 6.0 * c) / 6.0, p3 = (12.0 - 9.0 * b - 6.0 * c) / 6.0;
    const double q0 = (8.0 * b + 24.0 * c) / 6.0, q1 = (-12.0 * b - 48.0 * c) / 6.0, q2 = (6.0 * b + 30.0 * c) / 6.0, q3 = (-b - 6.0 * c) / 6.0;
    if (x < 1.0) return p0 + p2 * x * x + p3 * x * x * x;
    if (x < 2.0) return q0 + q1 * x + q2 * x * x + q3 * x * x * x;
    return 0.0;
}
}  // namespace

VSZIP_EXPORT int vszip_resample_table(int src_dim, int dst_dim, double shift, int32_t *left, float *coef4) {
    if (src_dim <= 0 || dst_dim < src_dim || !left || !coef4) return VSZIP_ERR_ARG;
    const double scale = (double)dst_dim / (double)src_dim;
    constexpr int kTaps = 4;  // ceil(2 * support), support 2, no widening when upscaling
    std::vector<double> row((size_t)src_dim);
    for (int i = 0; i < dst_dim; ++i) {
        std::fill(row.begin(), row.end(), 0.0);
        const double pos = (i + 0.5) / scale + shift;
        const double begin = std::floor(pos - kTaps / 2.0 + 0.5) + 0.5;
        double w[kTaps], total = 0.0;
        for (int k = 0; k < kTaps; ++k) {
            w[k] = bicubic_weight(begin + k - pos, 0.0, 0.5);  // VapourSynth's resize.Bicubic defaults: b = 0, c = 0.5
            total += w[k];
        }
        for (int k = 0; k < kTaps; ++k) {
            const double xpos = begin + k;
            double real = xpos < 0.0 ? -xpos : (xpos >= src_dim ? 2.0 * src_dim - xpos : xpos);
            real = std::min(std::max(real, 0.0), std::nextafter((double)src_dim, -INFINITY));
            row[(size_t)std::floor(real)] += w[k] / total;
        }
        int first = 0, last = 0;
        bool any = false;
        for (int j = 0; j < src_dim; ++j)
            if (row[j] != 0.0) {
                if (!any) first = j;
                last = j;
                any = true;
            }
        if (!any || last - first + 1 > kTaps) return VSZIP_ERR_UNSUPPORTED;
        // zimg aligns every row to the table's common width (4 wherever the line has 4 samples)
        const int width = std::min(kTaps, src_dim);
        const int l = std::min(first, src_dim - width);
        left[i] = l;
        for (int k = 0; k < kTaps; ++k) coef4[4 * i + k] = (l + k < src_dim) ? (float)row[(size_t)(l + k)] : 0.0f;
    }
    return VSZIP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Deband: the create-time tables of TempBuff.initFrameLuts (src/vapoursynth/deband.zig:162-319) with the generators of
// :336-431. One 32-bit state, mixed from seed, width, height and the frame count, serves everything in one serial
// order: per luma sample a grain dummy, one offset (two in mode 2) where the sample is at least one sample from the
// edges the mode looks at, and two grain dummies at every chroma site; then the luma and the chroma grain buffers (a
// plane without grain still consumes its values); then, for dynamic grain, one uniform value per frame. The tables hold
// the refEncode()d values themselves, not multiplied by a pitch: vszip_deband reads src[y +- dy][x +- dx].
// ---------------------------------------------------------------------------------------------------------
namespace {
struct DebandRng {
    uint32_t s;
    static double to_double(uint32_t v) {  // randToDouble: the state as the mantissa of a double in [1, 2), mapped to [-1, 1)
        uint64_t raw = ((uint64_t)v << 20) | ((uint64_t)v >> 12);
        raw |= 0x3ff0000000000000ull;
        double d;
        std::memcpy(&d, &raw, sizeof d);
        return (d - 1.0) * 2.0 - 1.0;
    }
    double old() {
        const uint32_t t = (((s << 13) ^ s) >> 17) ^ (s << 13) ^ s;
        s = (32u * t) ^ t;
        return to_double(s);
    }
    double uniform() {
        s = 1664525u * s + 1013904223u;
        return to_double(s);
    }
    double gaussian(double param) {
        for (;;) {
            double x, y, r2;
            do {
                x = uniform();
                y = uniform();
                r2 = x * x + y * y;
            } while (!(r2 <= 1.0 && r2 != 0.0));
            const double v = param * y * std::sqrt(-2.0 * std::log(r2) / r2);
            if (v > -1.0 && v < 1.0) return v;
        }
    }
    double real(int algo, double param) { return algo == 0 ? old() : (algo == 1 ? uniform() : gaussian(param)); }
    int32_t value(int algo, int32_t range, double param) { return (int32_t)std::round(real(algo, param) * (double)range); }
};

int deband_ref_encode(int32_t r) {  // neo_f3kdb's signed char: truncate, abs, truncate again: 128 comes back as -128
    const int t = (int8_t)(uint8_t)(uint32_t)r;
    const int a = t < 0 ? -t : t;
    return (int8_t)(uint8_t)a;
}

// Zig's {d}: integers without a point, other values in the shortest decimal form that reads back as the same double
void deband_fmt(char *out, size_t cap, double v) {
    if (v == std::floor(v) && std::fabs(v) < 1e15) {
        std::snprintf(out, cap, "%.0f", v);
        return;
    }
    for (int p = 1; p <= 17; ++p) {
        std::snprintf(out, cap, "%.*f", p, v);
        if (std::strtod(out, nullptr) == v) return;
    }
}

int deband_range_error(char *err, size_t cap, const char *key, double v, double lo, double hi) {
    if (err && cap) {
        char a[64], b[64], c[64];
        deband_fmt(a, sizeof a, v);
        deband_fmt(b, sizeof b, lo);
        deband_fmt(c, sizeof c, hi);
        std::snprintf(err, cap, "Deband: parameter \"%s=%s\" out of range [%s..%s].", key, a, b, c);
    }
    return VSZIP_ERR_ARG;
}
}  // namespace

VSZIP_EXPORT int vszip_deband_tables(const vszip_deband_cfg *cfg, vszip_deband_sizes *sizes, int8_t *luma, int8_t *chroma, void *grain_y, void *grain_c,
                                     uint32_t *grain_offsets, int32_t *max_offset, char *err, size_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!cfg) return VSZIP_ERR_ARG;
    // Data.setData's range checks on what this function is given, in its order and wording
    struct Check {
        const char *key;
        double v, lo, hi;
    } const checks[] = {
        {"sample_mode", (double)cfg->sample_mode, 1, 7},
        {"range", (double)cfg->range, 0, 255},
        {"random_param_ref", cfg->random_param_ref, 0, 255},
        {"random_param_grain", cfg->random_param_grain, 0, 255},
        {"random_algo_ref", (double)cfg->random_algo_ref, 0, 2},
        {"random_algo_grain", (double)cfg->random_algo_grain, 0, 2},
    };
    for (const Check &c : checks)
        if (!(c.v >= c.lo && c.v <= c.hi)) return deband_range_error(err, err_cap, c.key, c.v, c.lo, c.hi);
    const int w = cfg->width, h = cfg->height, ssw = cfg->ssw, ssh = cfg->ssh, mode = cfg->sample_mode;
    if (w <= 0 || h <= 0 || ssw < 0 || ssw > 4 || ssh < 0 || ssh > 4 || cfg->num_frames <= 0 || (int64_t)w * h > (int64_t)1 << 28) {
        if (err && err_cap) std::snprintf(err, err_cap, "Deband: bad geometry %dx%d, subsampling %d/%d, %d frames", w, h, ssw, ssh, cfg->num_frames);
        return VSZIP_ERR_ARG;
    }
    const bool dynamic = cfg->dynamic_grain != 0;
    const int cw = (w + (1 << ssw) - 1) >> ssw, ch = (h + (1 << ssh) - 1) >> ssh;
    const size_t items = (size_t)(((uint32_t)w + 255u) & 0xffffff80u) * (size_t)h, total = items * (dynamic ? 3 : 1);
    if (sizes) {
        sizes->luma_pairs = (size_t)w * h;
        sizes->chroma_pairs = (size_t)cw * ch;
        sizes->grain_items = total;
        sizes->grain_offsets = dynamic ? (size_t)cfg->num_frames : 0;
        sizes->chroma_w = cw;
        sizes->chroma_h = ch;
    }
    if (!luma) return VSZIP_OK;  // the query
    if (!chroma || (dynamic && !grain_offsets)) return VSZIP_ERR_ARG;

    const uint32_t w32 = (uint32_t)w, h32 = (uint32_t)h, nf32 = (uint32_t)cfg->num_frames;
    DebandRng r;
    r.s = 0x92D68CA2u - (uint32_t)cfg->seed;
    r.s ^= (w32 << 16) ^ h32;
    r.s ^= (nf32 << 16) ^ nf32;
    const int ar = cfg->random_algo_ref, ag = cfg->random_algo_grain, mask_w = (1 << ssw) - 1, mask_h = (1 << ssh) - 1;
    const double pr = cfg->random_param_ref, pg = cfg->random_param_grain;
    int largest = 0;
    for (int y = 0; y < h; ++y) {
        const int y_range = std::min(std::min(cfg->range, y), h - y - 1);
        int cx = 0;
        for (int x = 0; x < w; ++x) {
            (void)r.real(ag, pg);
            const int x_range = std::min(std::min(cfg->range, x), w - x - 1);
            const int cur = mode == 1 ? y_range : (mode == 3 ? x_range : std::min(x_range, y_range));
            int v1 = 0, v2 = 0;
            if (cur > 0) {
                v1 = deband_ref_encode(r.value(ar, cur, pr));
                if (mode == 2) v2 = deband_ref_encode(r.value(ar, cur, pr));
            }
            int8_t *l = luma + 2 * ((size_t)y * w + x);
            l[0] = (int8_t)v1;
            l[1] = (int8_t)v2;
            largest = std::max(largest, std::max(std::abs(v1), std::abs(v2)));
            if ((x & mask_w) == 0 && (y & mask_h) == 0) {
                int8_t *c = chroma + 2 * ((size_t)(y >> ssh) * cw + cx);
                c[0] = (int8_t)v1;
                c[1] = (int8_t)v2;
                (void)r.real(ag, pg);
                (void)r.real(ag, pg);
                ++cx;
            }
        }
    }
    if (max_offset) *max_offset = largest;
    void *const bufs[2] = {grain_y, grain_c};
    for (int i = 0; i < 2; ++i) {
        const bool on = cfg->is_float ? cfg->grain_f32[i] > 0.0f : cfg->grain_u16[i] > 0;
        if (!on || !bufs[i]) {
            for (size_t k = 0; k < total; ++k) (void)r.real(ag, pg);
        } else if (cfg->is_float) {
            float *g = static_cast<float *>(bufs[i]);
            const double range = (double)cfg->grain_f32[i];
            for (size_t k = 0; k < total; ++k) g[k] = (float)(r.real(ag, pg) * range);
        } else {
            int16_t *g = static_cast<int16_t *>(bufs[i]);
            const int32_t range = cfg->grain_u16[i];
            for (size_t k = 0; k < total; ++k) g[k] = (int16_t)r.value(ag, range, pg);
        }
    }
    if (dynamic) {
        const int32_t ic = (int32_t)items;
        for (int f = 0; f < cfg->num_frames; ++f) grain_offsets[f] = (uint32_t)(ic + r.value(1, ic, 1.0)) & 0xfffffff0u;
    }
    return VSZIP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// BilateralDither: the create-time derivation of src/vapoursynth/bilateral_dither.zig:151-209 (buildSlot :40-50) and
// the point lists of src/filters/bilateral_dither_subspl.zig:245-361. The derivation is f32 arithmetic in the
// reference's order. The lists: 23 per geometry, K points each, the first always (0, 0); under 32 points a 4-arm
// spiral whose start angle comes from minstd_rand0 and whose gaps an LCG fills, from 32 points on a scan of a
// toroidal void-and-cluster matrix at an offset from minstd_rand0, levels [0, trg) first and then one a pass.
// ---------------------------------------------------------------------------------------------------------
namespace {
constexpr int kBdLists = 23, kBdMaxPoints = 4096, kBdSpiralBelow = 32, kBdKernel = 9;

int bd_round_f32(double x) { return (int)std::nearbyintf((float)x); }  // fstb::round_int: to nearest, ties to even
int bd_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
uint32_t bd_lcg(uint32_t v) { return v * 1664525u + 1013904223u; }

struct BdMinstd {  // libstdc++'s default_random_engine with uniform_int_distribution<int>(0, n - 1)
    uint32_t s = 1;
    int dist(int n) {
        const uint32_t scaling = 2147483645u / (uint32_t)n, past = (uint32_t)n * scaling;
        uint32_t ret;
        do {
            s = (uint32_t)(((uint64_t)s * 16807u) % 2147483647u);
            ret = s - 1;
        } while (ret >= past);
        return (int)(ret / scaling);
    }
};

// a square matrix addressed modulo its size
template <typename T>
struct BdTorus {
    int n;
    std::vector<T> d;
    explicit BdTorus(int size) : n(size), d((size_t)size * size, T(0)) {}
    size_t at(int x, int y) const { return (size_t)(((y % n) + n) % n) * n + (size_t)(((x % n) + n) % n); }
    T get(int x, int y) const { return d[at(x, y)]; }
    T &ref(int x, int y) { return d[at(x, y)]; }
};

struct BdPos {
    int x, y;
};

// the first cell in scan order, among those of `color`, with the largest Gaussian sum over its neighbours of the same colour
BdPos bd_find_cluster(const BdTorus<uint16_t> &m, const double (&kern)[kBdKernel][kBdKernel], uint16_t color) {
    double best = -1.0;
    BdPos at{0, 0};
    constexpr int kh = (kBdKernel - 1) / 2;
    for (int y = 0; y < m.n; ++y)
        for (int x = 0; x < m.n; ++x) {
            if (m.get(x, y) != color) continue;
            double sum = 0.0;
            for (int j = -kh; j <= kh; ++j)
                for (int i = -kh; i <= kh; ++i)
                    if (m.get(x + i, y + j) == color) sum += kern[j + kh][i + kh];
            if (sum > best) {
                best = sum;
                at = BdPos{x, y};
            }
        }
    return at;
}

// the rank of every cell, 0 .. n * n - 1; depends on the size alone
BdTorus<uint16_t> bd_vnc_matrix(int n) {
    constexpr int kh = (kBdKernel - 1) / 2;
    double kern[kBdKernel][kBdKernel];
    const double inv2s2 = 1.0 / (2.0 * 1.5 * 1.5);
    for (int j = -kh; j <= kh; ++j)
        for (int i = -kh; i <= kh; ++i) kern[j + kh][i + kh] = std::exp(-(double)(i * i + j * j) * inv2s2);

    // a 10 % pattern by serpentine error diffusion, two passes
    BdTorus<uint16_t> base(n);
    BdTorus<double> err(n);
    int dir = 1;
    for (int pass = 0; pass < 2; ++pass)
        for (int y = 0; y < n; ++y) {
            for (int x = dir < 0 ? n - 1 : 0; x != (dir < 0 ? -1 : n); x += dir) {
                const double val = 0.1 + err.get(x, y);
                err.ref(x, y) = 0.0;
                const int q = bd_clamp(bd_round_f32(val), 0, 1);
                base.ref(x, y) = (uint16_t)q;
                const double e = val - (double)q;
                err.ref(x + dir, y) += e * 0.5;
                err.ref(x - dir, y + 1) += e * 0.25;
                err.ref(x, y + 1) += e * 0.25;
            }
            dir = -dir;
        }
    // move the tightest cluster's cell into the largest void until they are the same cell
    for (;;) {
        const BdPos c = bd_find_cluster(base, kern, 1);
        base.ref(c.x, c.y) = 0;
        const BdPos v = bd_find_cluster(base, kern, 0);
        base.ref(v.x, v.y) = 1;
        if (c.x == v.x && c.y == v.y) break;
    }
    int ones = 0;
    for (uint16_t v : base.d) ones += v == 1;
    BdTorus<uint16_t> vnc(n);
    {
        BdTorus<uint16_t> mat = base;
        for (int rank = ones; rank > 0;) {
            --rank;
            const BdPos c = bd_find_cluster(mat, kern, 1);
            mat.ref(c.x, c.y) = 0;
            vnc.ref(c.x, c.y) = (uint16_t)rank;
        }
    }
    {
        BdTorus<uint16_t> mat = base;
        for (int rank = ones; rank < n * n; ++rank) {
            const BdPos v = bd_find_cluster(mat, kern, 0);
            mat.ref(v.x, v.y) = 1;
            vnc.ref(v.x, v.y) = (uint16_t)rank;
        }
    }
    return vnc;
}

int bd_points_k(int radius, float subspl, double *actual_out) {
    const double s = (double)subspl, area = (double)((2 * radius - 1) * (2 * radius - 1));
    const double actual = s < 1e-3 ? (double)(2 * radius) : s;
    if (actual_out) *actual_out = actual;
    return bd_clamp(bd_round_f32(area / actual), 3, kBdMaxPoints);
}

// Zig's {d} of an f32: integers without a point, other values in the shortest decimal form that reads back as the same float
void bd_fmt(char *out, size_t cap, float v) {
    if (v == std::floor(v) && std::fabs(v) < 1e15f) {
        std::snprintf(out, cap, "%.0f", (double)v);
        return;
    }
    for (int p = 1; p <= 9; ++p) {
        std::snprintf(out, cap, "%.*g", p, (double)v);
        if (std::strtof(out, nullptr) == v) return;
    }
}

int bd_range_error(char *err, size_t cap, const char *key, float v, float lo, float hi) {
    if (err && cap) {
        char a[64], b[64];
        bd_fmt(a, sizeof a, v);
        bd_fmt(b, sizeof b, v < lo ? lo : hi);
        std::snprintf(err, cap, "BilateralDither: %s value %s is %s %s.", key, a, v < lo ? "below minimum" : "above maximum", b);
    }
    return VSZIP_ERR_ARG;
}
}  // namespace

VSZIP_EXPORT int vszip_bilateral_dither_derive(int is_float, int bits, int radius, float thr, float flat, float wmin, float subspl,
                                               vszip_bilateral_dither_cfg *out, char *err, size_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!out) return VSZIP_ERR_ARG;
    if (!is_float && (bits < 8 || bits > 16)) {
        if (err && err_cap) std::snprintf(err, err_cap, "BilateralDither: integer input must be 8..16 bit");
        return VSZIP_ERR_ARG;
    }
    // hz.getArray's checks, in the create function's order
    if (radius < 2 || radius > 16384) return bd_range_error(err, err_cap, "radius", (float)radius, 2, 16384);
    struct Check {
        const char *key;
        float v, lo, hi;
    } const checks[] = {{"thr", thr, 0, 65535}, {"flat", flat, 0, 1}, {"wmin", wmin, 0, 65535}, {"subspl", subspl, 0, 4096}};
    for (const Check &c : checks)
        if (!(c.v >= c.lo && c.v <= c.hi)) return bd_range_error(err, err_cap, c.key, c.v, c.lo, c.hi);
    const float scale = is_float ? 1.0f / 256.0f : (float)(1u << (bits - 8));
    const float unit = is_float ? 1.0f / 65535.0f : 1.0f;
    out->m = std::max(thr * scale, unit);
    const float t = thr * (1.0f - flat);
    out->wmax = std::max(t * scale, unit);
    out->subsampled = subspl >= 4.0f || (double)subspl < 1e-3;
    out->K = out->subsampled ? bd_points_k(radius, subspl, nullptr) : 0;
    const float n = out->subsampled ? (float)out->K : (float)((2 * radius - 1) * (2 * radius - 1));
    const float ww = wmin * out->wmax;
    out->sum_w_min = std::max(ww * n, unit);
    return VSZIP_OK;
}

VSZIP_EXPORT int vszip_bilateral_dither_points(int radius, float subspl, int16_t *points, size_t capacity, int32_t *K_out) {
    if (radius < 2 || radius > 16384 || !(subspl >= 0.0f && subspl <= 4096.0f)) return VSZIP_ERR_ARG;
    double actual;
    const int K = bd_points_k(radius, subspl, &actual);
    if (K_out) *K_out = K;
    if (!points) return VSZIP_OK;  // the query
    if (capacity < (size_t)kBdLists * K) return VSZIP_ERR_ARG;
    const int r = radius, win = 2 * r - 1;
    const int n = bd_clamp(win * 3 / 2, 16, 32);
    BdTorus<uint16_t> vnc(K >= kBdSpiralBelow ? n : 1);
    if (K >= kBdSpiralBelow) vnc = bd_vnc_matrix(n);  // once a call
    BdMinstd ms_a, ms_x, ms_y;
    uint32_t rnd = 1;
    // (K < 32 means win * win < 4096 * 32; K >= 32 visits the window cell by cell)
    std::vector<char> done((size_t)win * win);
    const double pi = 3.1415926535897932384626433832795;
    for (int lc = 0; lc < kBdLists; ++lc) {
        int16_t *cur = points + (size_t)lc * K * 2;
        std::fill(done.begin(), done.end(), 0);
        cur[0] = cur[1] = 0;
        done[(size_t)(r - 1) + (size_t)(r - 1) * win] = 1;
        int cnt = 1;
        auto put = [&](int x, int y) {
            const size_t da = (size_t)(x + r - 1) + (size_t)(y + r - 1) * win;
            if (done[da]) return;
            cur[2 * cnt] = (int16_t)x;
            cur[2 * cnt + 1] = (int16_t)y;
            done[da] = 1;
            ++cnt;
        };
        if (K < kBdSpiralBelow) {
            const double angle_base = (double)ms_a.dist(kBdLists) * (pi * 0.5 / (double)kBdLists);
            const int arm_dir = 1 - (lc & 2), narm = 4, npa = (K - 1) / narm;
            const double amul = 2.0 * pi / (double)narm * (double)arm_dir;
            for (int p = 0; p < npa; ++p) {
                const double posd = std::pow((double)p / (double)npa, 3.0 / 5.0);
                for (int a = 0; a < narm; ++a) {
                    const double ang = angle_base + (posd * 2.0 + (double)a) * amul;
                    const int x = bd_round_f32(std::cos(ang) * posd * (double)(r - 1));
                    const int y = bd_round_f32(std::sin(ang) * posd * (double)(r - 1));
                    if (x > -r && x < r && y > -r && y < r) put(x, y);
                }
            }
            while (cnt < K) {
                rnd = bd_lcg(rnd);
                const int x = (int)((rnd >> 8) % (uint32_t)win) - (r - 1);
                rnd = bd_lcg(rnd);
                const int y = (int)((rnd >> 8) % (uint32_t)win) - (r - 1);
                put(x, y);
            }
        } else {
            const int ofs_x = ms_x.dist(win), ofs_y = ms_y.dist(win);
            int lo = 0, hi = (int)std::floor((double)(n * n) / actual);
            while (cnt < K) {
                for (int y = 0; y < win && cnt < K; ++y)
                    for (int x = 0; x < win && cnt < K; ++x) {
                        const int v = vnc.get(x + ofs_x, y + ofs_y);
                        if (v >= lo && v < hi) put(x - (r - 1), y - (r - 1));
                    }
                lo = hi;
                ++hi;
            }
        }
    }
    return VSZIP_OK;
}

// ---- Compress: the quantiser tables of one clip (QuantTables.buildMpeg2 / buildJpeg, src/filters/compress.zig:80-103) and the
// create-time checks of compressCreate (src/vapoursynth/compress.zig:77-110), in its order ----
namespace {
// natural raster order: the MPEG-1/2 default intra matrix (luma and chroma), the JPEG Annex K luminance and chrominance tables
const int kMpegIntra[64] = {8,  16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
                            22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83};
const int kJpegBase[2][64] = {{16, 11, 10, 16, 24, 40, 51, 61,  12, 12, 14, 19, 26, 58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
                              {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

int compress_error(char *err, size_t cap, const char *text) {
    if (err && cap) std::snprintf(err, cap, "Compress: %s", text);
    return VSZIP_ERR_ARG;
}
}  // namespace

VSZIP_EXPORT int vszip_compress_tables(int codec, int qscale, int dc_prec, int quality, struct vszip_compress_tables *out, char *err, size_t err_cap) {
    if (!out) return compress_error(err, err_cap, "out must not be NULL");
    if (codec < 0 || codec > 1) return compress_error(err, err_cap, "codec must be 0 (mpeg2) or 1 (jpeg).");
    out->codec = codec;
    out->dc_q = 64;
    out->dc_scale = 8;
    if (codec == 0) {
        if (qscale < 1 || qscale > 31) return compress_error(err, err_cap, "qscale must be between 1 and 31.");
        if (dc_prec < 0 || dc_prec > 3) return compress_error(err, err_cap, "dc_prec must be between 0 and 3.");
        for (int i = 0; i < 64; ++i) {
            const int den = (qscale << 1) * kMpegIntra[i];
            out->qmul[0][i] = out->qmul[1][i] = (int32_t)(((int64_t)2 << 21) / den);
            out->deq[0][i] = out->deq[1][i] = den;
        }
        out->dc_scale = 8 >> dc_prec;
        out->dc_q = out->dc_scale << 3;
    } else {
        if (quality < 1 || quality > 100) return compress_error(err, err_cap, "quality must be between 1 and 100.");
        const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
        for (int p = 0; p < 2; ++p)
            for (int i = 0; i < 64; ++i) {
                const int q = std::min(std::max((kJpegBase[p][i] * scale + 50) / 100, 1), 255);
                out->deq[p][i] = q;
                out->qmul[p][i] = (int32_t)(((int64_t)1 << 21) / (8 * q));
            }
    }
    return VSZIP_OK;
}

// ---- ColorMap: the 256-entry table of one palette (colorMapCreate, src/vapoursynth/color_map.zig:92-103), with its roundings ----
VSZIP_EXPORT int vszip_color_map_lut(const float *r, const float *g, const float *b, int len, uint8_t lut[3][256], char *err, size_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!r || !g || !b || !lut) {
        if (err && err_cap) std::snprintf(err, err_cap, "ColorMap: r, g, b and lut must not be NULL");
        return VSZIP_ERR_ARG;
    }
    if (len < 1 || len > (1 << 24)) {
        if (err && err_cap) std::snprintf(err, err_cap, "ColorMap: len = %d, a palette has 1 .. 16777216 points", len);
        return VSZIP_ERR_ARG;
    }
    const float *pal[3] = {r, g, b};
    const float lenm1 = (float)(len - 1);
    for (int i = 0; i < 256; ++i) {
        const volatile float scaled = (float)i * lenm1;  // volatile: every operation of the interpolation is rounded to f32 on its own, whatever
        const float p = scaled / 255.0f;                 // the compiler's contraction rule is (the reference's multiply and add are not fused)
        const int lo = (int)std::floor(p), hi = std::min(lo + 1, len - 1);
        const float frac = p - (float)lo;
        for (int c = 0; c < 3; ++c) {
            const volatile float d = pal[c][hi] - pal[c][lo];
            const volatile float prod = d * frac;
            const volatile float v = pal[c][lo] + prod;
            const float t = std::fmaf(v, 255.0f, 0.5f);  // the reference's @mulAdd: one rounding
            if (!(t > -1.0f && t < 256.0f)) {
                if (err && err_cap) std::snprintf(err, err_cap, "ColorMap: %c: table entry %d (palette points %d and %d) gives %g, outside 0..255", "rgb"[c], i, lo, hi, (double)t);
                return VSZIP_ERR_ARG;
            }
            lut[c][i] = (uint8_t)(int)t;  // truncation towards zero
        }
    }
    return VSZIP_OK;
}

// ---- Depth: the argument checks of vszip_depth, in its order (tests/depth_ref.py check_args restates them) ----
VSZIP_EXPORT int vszip_depth_check(int bits_in, int bits_out, int dither, int full_range, const vszip_depth_plane *planes, int nplanes, char *err, size_t err_cap) {
    char none[1];
    if (!err || !err_cap) err = none, err_cap = sizeof none;
    err[0] = 0;
    auto fail = [](int code, int) { return code; };
    if (bits_in < 8 || bits_in > 16) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "Depth: bits_in %d is outside 8..16", bits_in));
    if (bits_out < 8 || bits_out > 16) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "Depth: bits_out %d is outside 8..16", bits_out));
    if (dither != 0 && dither != 1) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "Depth: dither %d is neither 0 (none) nor 1 (error diffusion)", dither));
    if (!planes || nplanes <= 0) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "Depth: no planes"));
    long long rows = 0;
    for (int i = 0; i < nplanes; ++i) {
        const vszip_depth_plane &s = planes[i];
        if (!s.src || !s.dst) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "Depth: plane %d: src and dst must not be NULL", i));
        if (s.w < 1 || s.h < 1 || s.src_stride < s.w || s.dst_stride < s.w || std::max(s.src_stride, s.dst_stride) > 2147483647)
            return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "Depth: plane %d: bad geometry %dx%d, pitches %lld -> %lld", i, (int)s.w, (int)s.h, (long long)s.src_stride,
                                                     (long long)s.dst_stride));
        if (full_range && s.chroma)
            return fail(VSZIP_ERR_UNSUPPORTED, std::snprintf(err, err_cap, "Depth: plane %d: full-range chroma is not built (DESIGN.md section 1)", i));
        rows += s.h;
    }
    if (rows > 2147483647 / 2) return fail(VSZIP_ERR_UNSUPPORTED, std::snprintf(err, err_cap, "Depth: %lld rows are more than one call numbers", rows));
    return VSZIP_OK;
}

// ---- DepthFmt: the argument checks of vszip_depth_fmt, in its order (tests/depth_fmt_ref.py check_args restates them) ----
VSZIP_EXPORT int vszip_depth_fmt_check(int dtype_in, int bits_in, int dtype_out, int bits_out, int dither, int full_range, const vszip_depth_plane *planes,
                                       int nplanes, char *err, size_t err_cap) {
    namespace df = depth_fmt;
    char none[1];
    if (!err || !err_cap) err = none, err_cap = sizeof none;
    err[0] = 0;
    auto fail = [](int code, int) { return code; };
    const struct {
        const char *name;
        int dtype, bits;
    } side[2] = {{"in", dtype_in, bits_in}, {"out", dtype_out, bits_out}};
    for (const auto &s : side)
        if (!df::known_dtype(s.dtype))
            return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "DepthFmt: dtype_%s %d is none of VSZIP_U8, VSZIP_U16, VSZIP_F16, VSZIP_F32", s.name, s.dtype));
    for (const auto &s : side)
        if (!df::bits_fit(s.dtype, s.bits)) {
            const int lo = df::bits_lo(s.dtype), hi = df::bits_hi(s.dtype);
            if (lo == hi) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "DepthFmt: bits_%s %d does not fit %s (%d)", s.name, s.bits, df::dtype_name(s.dtype), lo));
            return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "DepthFmt: bits_%s %d does not fit %s (%d..%d)", s.name, s.bits, df::dtype_name(s.dtype), lo, hi));
        }
    const bool in_float = df::is_float(dtype_in), out_float = df::is_float(dtype_out);
    if (!in_float && !out_float) return vszip_depth_check(bits_in, bits_out, dither, full_range, planes, nplanes, err, err_cap);  // vszip_depth itself
    if (dither != 0 && dither != 1) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "DepthFmt: dither %d is neither 0 (none) nor 1 (error diffusion)", dither));
    if (dither && out_float)
        return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "DepthFmt: error diffusion needs an integer destination, dtype_out is %s", df::dtype_name(dtype_out)));
    if (!planes || nplanes <= 0) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "DepthFmt: no planes"));
    long long rows = 0;
    for (int i = 0; i < nplanes; ++i) {
        const vszip_depth_plane &s = planes[i];
        if (!s.src || !s.dst) return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "DepthFmt: plane %d: src and dst must not be NULL", i));
        if (s.w < 1 || s.h < 1 || s.src_stride < s.w || s.dst_stride < s.w || std::max(s.src_stride, s.dst_stride) > 2147483647)
            return fail(VSZIP_ERR_ARG, std::snprintf(err, err_cap, "DepthFmt: plane %d: bad geometry %dx%d, pitches %lld -> %lld", i, (int)s.w, (int)s.h,
                                                     (long long)s.src_stride, (long long)s.dst_stride));
        if (dither && df::range_of(bits_out, full_range != 0, s.chroma != 0).off != 0)
            return fail(VSZIP_ERR_UNSUPPORTED, std::snprintf(err, err_cap, "DepthFmt: plane %d: error diffusion from float with an offset (%s) is not built (DESIGN.md section 1)", i,
                                                             full_range ? "chroma" : "limited range"));
        rows += s.h;
    }
    if (rows > 2147483647 / 2) return fail(VSZIP_ERR_UNSUPPORTED, std::snprintf(err, err_cap, "DepthFmt: %lld rows are more than one call numbers", rows));
    return VSZIP_OK;
}
