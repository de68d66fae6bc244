// vszip.Deband on gfx950 (src/filters/deband_int.zig, deband_float.zig as called by src/vapoursynth/deband.zig): per output
// sample two or four reads of the source at offsets that a per-clip table holds per sample (up to +-128 samples; +-15 by
// default), a threshold decision or a soft blend, grain from a second per-clip table, a clamp. A random gather beside three
// streams (source, table, grain) and one store stream.
//
// Tables hold the reference's raw (val1, val2) pairs, not flat offsets; pairs_of() (deband_math.hpp) turns them into the two
// sample pairs of the mode for this plane's subsampling, and every sampled coordinate is clamped, so no table can make a kernel
// read outside [0, w) x h. For tables from vszip_deband_tables the clamp never changes a coordinate.
//
// Work split. A workgroup of 256 threads makes a 64 x 32 tile; a thread makes four consecutive samples of a row, twice. Two
// gather paths, same arithmetic (sample_int / sample_float):
//   tile    the tile and a halo of H samples on every side (H = 16 or 32, by the call's max_offset) are staged in LDS, clipped
//           to the plane; gathers read LDS, coordinates clamped into what was staged;
//   direct  gathers read global memory, coordinates clamped into the plane; any max_offset.
// Sample mode 7 looks up the normalised gradient angle at the sample and at its four references: a first kernel writes the
// angle of every sample of a plane (a Sobel at distance 20, coordinates clamped to the plane) into scratch, pitch w; the
// reference's 128-sample padded copy is unnecessary because every lookup lands inside the plane.
//
// Vector accesses (four samples: source, table pairs, grain, destination) need bases and pitches that are multiples of four
// samples, and are made for whole groups inside [0, w) only; anything else goes sample by sample with the same bits. The LDS
// staging loads whole groups of four and may cover pitch padding (inside h x stride), which lands in columns nothing reads.
#include <algorithm>
#include <cstdlib>

#include "deband_body.hpp"
#include "depth.hpp"
#include "plane_table.hpp"

namespace {

using deband::DebPlane;
using deband::kTW;
using deband::kTH;
using deband::kThreads;
using deband::kHaloSmall;
using deband::kHaloLarge;

// An entry is 96 bytes; 96 of them are 9 KiB of kernel argument, what a MosquitoNR launch carries. 96 planes are 32 YUV frames.
constexpr int kDebPlanes = 96;
struct DebParams : PlaneTable<DebPlane, kDebPlanes> {
    float angle_boost, max_angle;
    int blur_first;
};

#if defined(__HIPCC__)
template <typename T>
__global__ __launch_bounds__(kThreads) void deband_angle_kernel(const DebParams prm) {
    const int b = blockIdx.x;
    const DebPlane &pl = prm.p[vszip_find_plane(prm, b)];
    const int tile = b - pl.block0, ty = tile / pl.tiles_x, tx = tile - ty * pl.tiles_x;
    deband::angle_tile<T>(pl, tx, ty, threadIdx.x);
}

// HALO == 0: the direct path
template <typename T, int MODE, int HALO>
__global__ __launch_bounds__(kThreads) void deband_kernel(const DebParams prm) {
    __shared__ T tileS[HALO ? deband::TileShape<HALO>::kPitch * deband::TileShape<HALO>::kRows : 1];
    const int b = blockIdx.x;
    const DebPlane &pl = prm.p[vszip_find_plane(prm, b)];
    const int tile = b - pl.block0, ty = tile / pl.tiles_x, tx = tile - ty * pl.tiles_x;
    if constexpr (HALO != 0) {
        deband::stage_tile<T, HALO>(pl, tx * kTW, ty * kTH, threadIdx.x, tileS);
        __syncthreads();
    }
    deband::make_tile<T, MODE, HALO>(pl, prm.angle_boost, prm.max_angle, prm.blur_first, tx * kTW, ty * kTH, threadIdx.x, tileS);
}

template <typename T, int HALO>
void launch_mode(int mode, int blocks, hipStream_t stream, const DebParams &t) {
    switch (mode) {
        case 1: hipLaunchKernelGGL((deband_kernel<T, 1, HALO>), dim3(blocks), dim3(kThreads), 0, stream, t); break;
        case 2: hipLaunchKernelGGL((deband_kernel<T, 2, HALO>), dim3(blocks), dim3(kThreads), 0, stream, t); break;
        case 3: hipLaunchKernelGGL((deband_kernel<T, 3, HALO>), dim3(blocks), dim3(kThreads), 0, stream, t); break;
        case 4: hipLaunchKernelGGL((deband_kernel<T, 4, HALO>), dim3(blocks), dim3(kThreads), 0, stream, t); break;
        case 5: hipLaunchKernelGGL((deband_kernel<T, 5, HALO>), dim3(blocks), dim3(kThreads), 0, stream, t); break;
        case 6: hipLaunchKernelGGL((deband_kernel<T, 6, HALO>), dim3(blocks), dim3(kThreads), 0, stream, t); break;
        default: hipLaunchKernelGGL((deband_kernel<T, 7, HALO>), dim3(blocks), dim3(kThreads), 0, stream, t); break;
    }
}

template <typename T>
void launch(int mode, int halo, int blocks, hipStream_t stream, const DebParams &t) {
    if (mode == 7) hipLaunchKernelGGL(deband_angle_kernel<T>, dim3(blocks), dim3(kThreads), 0, stream, t);
    if (halo == kHaloSmall)
        launch_mode<T, kHaloSmall>(mode, blocks, stream, t);
    else if (halo == kHaloLarge)
        launch_mode<T, kHaloLarge>(mode, blocks, stream, t);
    else
        launch_mode<T, 0>(mode, blocks, stream, t);
}
#endif  // __HIPCC__

int range_error(vszip_ctx *ctx, const char *key, double v, int lo, int hi) {
    // Maps.getValue, src/helper.zig:419-429 ({d} prints 2 for 2.0)
    char num[64];
    if (v == std::floor(v) && std::fabs(v) < 1e15)
        snprintf(num, sizeof num, "%.0f", v);
    else
        for (int p = 1; p <= 17; ++p) {
            snprintf(num, sizeof num, "%.*f", p, v);
            if (strtod(num, nullptr) == v) break;
        }
    return vszip_set_error(ctx, VSZIP_ERR_ARG, "Deband: parameter \"%s=%s\" out of range [%d..%d].", key, num, lo, hi);
}

// vszip_deband_lowbit: the planes are at `bits` and pass through two 16-bit intermediates of the group's scratch
struct LowBit {
    int bits, full_range;
};

int deband_run(vszip_ctx *ctx, int dtype, const vszip_plane *planes, const vszip_deband_plane *per, int nplanes, int sample_mode, int blur_first, float angle_boost,
               float max_angle, int max_offset, const LowBit *low) {
    if (!planes || !per || nplanes <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Deband: no planes");
    if (dtype != VSZIP_U16 && dtype != VSZIP_F32)
        return vszip_set_error(ctx, VSZIP_ERR_ARG, "Deband: 16-bit integer or 32-bit float planes only (clips under 16 bits go through vszip_deband_lowbit).");
    if (sample_mode < 1 || sample_mode > 7) return range_error(ctx, "sample_mode", sample_mode, 1, 7);
    if (!(angle_boost >= 0.0f && angle_boost <= 65535.0f)) return range_error(ctx, "angle_boost", angle_boost, 0, 65535);
    if (!(max_angle >= 0.0f && max_angle <= 1.0f)) return range_error(ctx, "max_angle", max_angle, 0, 1);
    if (max_offset < 0 || max_offset > 128) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Deband: max_offset %d is outside 0..128", max_offset);
    for (int i = 0; i < nplanes; ++i) {
        const vszip_plane &s = planes[i];
        const vszip_deband_plane &d = per[i];
        if (!s.src || !s.dst || !d.offsets || s.w <= 0 || s.h <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Deband: plane %d: src, dst and offsets must not be NULL", i);
        if (d.ssw < 0 || d.ssw > 4 || d.ssh < 0 || d.ssh > 4) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Deband: plane %d: subsampling %d/%d is outside 0..4", i, d.ssw, d.ssh);
        if (d.offsets_pitch < s.w || (d.grain && d.grain_pitch < s.w)) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Deband: plane %d: a table pitch is below the plane's width", i);
    }
    // under 16 bits: the conversions around the filter, plane i of the caller -> intermediate and intermediate -> plane i (pointers per group)
    std::vector<vszip_depth_plane> up, down;
    std::vector<vszip_plane> mid;
    if (low) {
        up.resize(nplanes), down.resize(nplanes), mid.resize(nplanes);
        for (int i = 0; i < nplanes; ++i) {
            const vszip_plane &s = planes[i];
            const ptrdiff_t pitch = ((ptrdiff_t)s.w + 7) & ~(ptrdiff_t)7;  // whole 16-byte groups
            up[i] = vszip_depth_plane{s.src, s.src_stride, nullptr, pitch, s.w, s.h, 0};
            down[i] = vszip_depth_plane{nullptr, pitch, s.dst, s.dst_stride, s.w, s.h, 0};
            mid[i] = vszip_plane{};
            mid[i].src_stride = mid[i].dst_stride = pitch;
            mid[i].w = s.w, mid[i].h = s.h;
        }
        char msg[256];
        // the conversions' own checks (the caller's pitches), with a stand-in for the intermediates that do not exist yet
        for (int i = 0; i < nplanes; ++i) up[i].dst = msg, down[i].src = msg;
        int bad = vszip_depth_check(low->bits, 16, 0, low->full_range, up.data(), nplanes, msg, sizeof msg);
        if (bad == VSZIP_OK) bad = vszip_depth_check(16, low->bits, 1, low->full_range, down.data(), nplanes, msg, sizeof msg);
        if (bad != VSZIP_OK) return vszip_set_error(ctx, bad, "%s", msg);
        planes = nullptr;  // from here on: up / mid / down
    }
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));

    // the gather path: 0 by max_offset, 1 the LDS tile wherever its halo covers max_offset, 2 always global memory
    const int path = ctx->opt.deband_path;
    int halo = 0;
    if (path != 2 && max_offset <= kHaloLarge) halo = max_offset <= kHaloSmall ? kHaloSmall : kHaloLarge;

    // plane groups whose scratch fits the caps (a plane alone may exceed them: planes are never split). Mode 7: the angle planes, at most
    // VSZIP_DEBAND_SCRATCH_MIB. Under 16 bits: two intermediates a plane, at most VSZIP_DEBAND_LOWBIT_SCRATCH_MIB, and the carry rows of the
    // conversion back.
    const size_t cap = (size_t)std::max(ctx->opt.deband_scratch_mib, 1) << 20, cap_low = (size_t)std::max(ctx->opt.deband_lowbit_scratch_mib, 1) << 20;
    DebParams prm;
    prm.angle_boost = angle_boost;
    prm.max_angle = max_angle;
    prm.blur_first = blur_first != 0;
    for (int done = 0; done < nplanes;) {
        int n = nplanes - done;
        scratch::Layout lay;
        std::vector<scratch::Region<float>> angle;  // the group's angle planes, a multiple of 256 bytes each
        std::vector<scratch::Region<uint16_t>> inter;  // the group's intermediates, two a plane
        std::vector<scratch::Region<float>> carry;
        char *base = nullptr;
        if (sample_mode == 7 || low) {
            n = 0;
            size_t angle_bytes = 0, inter_bytes = 0;
            while (done + n < nplanes) {
                const int w = low ? mid[done + n].w : planes[done + n].w, h = low ? mid[done + n].h : planes[done + n].h;
                scratch::Layout with = lay;
                scratch::Region<float> a;
                scratch::Region<uint16_t> ia, ib;
                size_t angle_with = angle_bytes, inter_with = inter_bytes;
                if (sample_mode == 7) {
                    a = with.take<float>((size_t)w * h);
                    with.align_to(256);
                    angle_with = (angle_bytes + a.bytes() + 255) / 256 * 256;
                }
                if (low) {
                    const size_t count = (size_t)mid[done + n].src_stride * h;
                    ia = with.take<uint16_t>(count, 256);
                    ib = with.take<uint16_t>(count, 256);
                    with.align_to(256);
                    inter_with += 2 * ((ia.bytes() + 255) / 256 * 256);
                }
                if (n > 0 && ((sample_mode == 7 && angle_with > cap) || (low && inter_with > cap_low))) break;
                lay = with;
                angle_bytes = angle_with, inter_bytes = inter_with;
                if (sample_mode == 7) angle.push_back(a);
                if (low) inter.push_back(ia), inter.push_back(ib);
                ++n;
            }
            if (low) vszip_depth_take_carry(ctx, lay, down.data() + done, n, 1, carry);
            const int rc = vszip_reserve_scratch(ctx, lay, &base);
            if (rc != VSZIP_OK) return rc;
        }
        if (low) {
            for (int j = 0; j < n; ++j) {
                uint16_t *a = inter[2 * j].in(base), *b = inter[2 * j + 1].in(base);
                up[done + j].dst = a, mid[done + j].src = a, mid[done + j].dst = b, down[done + j].src = b;
            }
            const int rc = vszip_depth_queue(ctx, up.data() + done, n, low->bits, 16, 0, low->full_range, std::vector<scratch::Region<float>>(n), base);
            if (rc != VSZIP_OK) return rc;
        }
        const vszip_plane *group = low ? mid.data() : planes;
        const int rc = vszip_for_each_table(
            ctx, prm, n,
            [&](DebPlane &d, int j) -> int {
                const int i = done + j;
                const vszip_plane &s = group[i];
                const vszip_deband_plane &q = per[i];
                d.src = s.src;
                d.dst = s.dst;
                d.off = q.offsets;
                d.grain = q.grain;
                d.angle = nullptr;
                if (sample_mode == 7) d.angle = angle[j].in(base);
                d.sstride = (int)s.src_stride;
                d.dstride = (int)s.dst_stride;
                d.ostride = (int)q.offsets_pitch;
                d.gstride = (int)q.grain_pitch;
                d.w = s.w;
                d.h = s.h;
                d.tiles_x = (s.w + kTW - 1) / kTW;
                d.thr = q.thr;
                d.thr1 = q.thr1;
                d.thr2 = q.thr2;
                d.lo = q.lo;
                d.hi = q.hi;
                d.ssw = (short)q.ssw;
                d.ssh = (short)q.ssh;
                return d.tiles_x * ((s.h + kTH - 1) / kTH);
            },
            [&](const DebParams &t, int blocks, int) {
                vszip_probe_scope probe(ctx);
                if (dtype == VSZIP_U16)
                    launch<uint16_t>(sample_mode, halo, blocks, ctx->stream, t);
                else
                    launch<float>(sample_mode, halo, blocks, ctx->stream, t);
                return VSZIP_OK;
            });
        if (rc != VSZIP_OK) return rc;
        if (low) {
            const int rc2 = vszip_depth_queue(ctx, down.data() + done, n, 16, low->bits, 1, low->full_range, carry, base);
            if (rc2 != VSZIP_OK) return rc2;
        }
        done += n;
    }
    return VSZIP_OK;
}

}  // namespace

VSZIP_EXPORT int vszip_deband(vszip_ctx *ctx, int dtype, const vszip_plane *planes, const vszip_deband_plane *per, int nplanes, int sample_mode, int blur_first,
                              float angle_boost, float max_angle, int max_offset) {
    if (!ctx) return VSZIP_ERR_ARG;
    return deband_run(ctx, dtype, planes, per, nplanes, sample_mode, blur_first, angle_boost, max_angle, max_offset, nullptr);
}

VSZIP_EXPORT int vszip_deband_lowbit(vszip_ctx *ctx, int bits, int full_range, const vszip_plane *planes, const vszip_deband_plane *per, int nplanes, int sample_mode,
                                     int blur_first, float angle_boost, float max_angle, int max_offset) {
    if (!ctx) return VSZIP_ERR_ARG;
    if (bits < 8 || bits > 15) return vszip_set_error(ctx, VSZIP_ERR_ARG, "Deband: bits %d is outside 8..15 (16-bit clips go through vszip_deband)", bits);
    const LowBit low{bits, full_range};
    return deband_run(ctx, VSZIP_U16, planes, per, nplanes, sample_mode, blur_first, angle_boost, max_angle, max_offset, &low);
}
