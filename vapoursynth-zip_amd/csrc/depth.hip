// vszip_depth on gfx950: integer depth conversion as zimg's resize.Point does it with dither_type none and error_diffusion, the step that
// hz.bitDepth (src/helper.zig:470-494) asks the host's resizer for around Deband and XPSNR. The arithmetic is depth_plan.hpp's
// convert_none / diffuse: f32, every operation rounded on its own (the library is built with contraction off).
//
// none. One streaming pass: a lane owns a group of 16 samples (8 when both planes are 16-bit), 16-byte loads and stores, a workgroup a band
// of rows walked in raster order (row_units.hpp). Frames whose bases or pitches (in bytes) are no multiples of 16 go sample by sample.
//
// error diffusion. The recurrence is serial: (y, x) needs (y, x - 1) and (y - 1, x - 1 .. x + 1). One workgroup walks one plane as a skewed
// wavefront, by the schedule of depth_plan.hpp: lane l of a wave owns row y0 + l and is at column t - 2 l at step t, so the lane above is
// two columns ahead and hands its fresh error down by a wave_shr:1 DPP move; the lane keeps the last three in registers (top[x - 1],
// top[x], top[x + 1]). The waves of the workgroup take consecutive 64-row bands, each kLagChunks chunks of 64 steps behind the one above;
// the seam row's errors go through an LDS ring (the last wave's: a whole row, the carry row, in LDS up to 4096 columns and in the
// context's scratch beyond), fetched one column a lane at the start of a chunk and dealt to lane 0 by v_readlane. One __syncthreads() a
// chunk; every wave executes plan.chunks of them, a function of w and h alone. No workgroup waits for another.
// A lane loads its row's samples eight at a time, a group ahead of use, into a shift register of dwords, and collects eight outputs in
// another before it stores them; groups that are not whole, or planes whose bases or pitches are no multiples of 16 bytes, go sample by
// sample at the same moments. Nothing outside [0, w) x h is read or written.
#include <algorithm>
#include <climits>
#include <type_traits>

#include "depth.hpp"
#include "row_units.hpp"

namespace {

namespace dp = depth_plan;

// An entry is 56 bytes; 128 of them are 7 KiB of kernel argument.
constexpr int kDepthPlanes = 128;
struct DepthPlane {
    const void *src;
    void *dst;
    float *carry;  // error diffusion: the carry row in scratch (planes that need one)
    int sstride, dstride, w, h;
    short svec, dvec;  // base and pitch are multiples of 16 bytes
    short rows;        // none: rows a workgroup
    int block0;
};
struct DepthParams : PlaneTable<DepthPlane, kDepthPlanes> {
    float scale, peak;
};

#if defined(__HIPCC__)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- none -----------------------------------------------------------------------------------------------------------------------------
template <typename Tin, typename Tout>
__global__ __launch_bounds__(kRowUnitThreads) void depth_none_kernel(const DepthParams prm) {
    constexpr int V = (sizeof(Tin) == 1 || sizeof(Tout) == 1) ? 16 : 8;  // samples a lane: 16 bytes of the narrower plane
    typedef Tin VI __attribute__((ext_vector_type(V), aligned(16)));
    typedef Tout VO __attribute__((ext_vector_type(V), aligned(16)));
    const int wg = blockIdx.x;
    const DepthPlane &f = prm.p[vszip_find_plane(prm, wg)];
    const int y0 = (wg - f.block0) * f.rows, rows = min((int)f.rows, f.h - y0), w = f.w, ss = f.sstride, ds = f.dstride;
    const Tin *s = static_cast<const Tin *>(f.src) + (size_t)y0 * ss;
    Tout *d = static_cast<Tout *>(f.dst) + (size_t)y0 * ds;
    const float scale = prm.scale, peak = prm.peak;
    int x0 = 0;
    if (f.svec && f.dvec) {
        const int nv = w / V;
        for_each_row_unit(rows, nv, [&](int row, int i) {
            const VI v = *(reinterpret_cast<const VI *>(s + (size_t)row * ss) + i);
            VO o;
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = (Tout)dp::convert_none((float)v[e], scale, peak);
            __builtin_nontemporal_store(o, reinterpret_cast<VO *>(d + (size_t)row * ds) + i);
        });
        x0 = nv * V;
    }
    for_each_row_unit(rows, w - x0, [&](int row, int i) {
        const size_t x = (size_t)x0 + i;
        d[(size_t)row * ds + x] = (Tout)dp::convert_none((float)s[(size_t)row * ss + x], scale, peak);
    });
}

// ---- error diffusion ------------------------------------------------------------------------------------------------------------------
// A sample as the bits a Group keeps, and those bits as the f32 the arithmetic starts from: integers by value, float planes (the
// instantiations of depth_fmt.hip: f32, and f16 widened at pop) by their bit pattern.
template <typename T>
__device__ __forceinline__ uint32_t sample_bits(T v) {
    if constexpr (std::is_integral_v<T>)
        return (uint32_t)v;
    else if constexpr (sizeof(T) == 4)
        return __float_as_uint(v);
    else
        return (uint32_t)__builtin_bit_cast(uint16_t, v);
}
template <typename T>
__device__ __forceinline__ float sample_value(uint32_t bits) {
    if constexpr (std::is_integral_v<T>)
        return (float)bits;
    else if constexpr (sizeof(T) == 4)
        return __uint_as_float(bits);
    else
        return (float)__builtin_bit_cast(T, (uint16_t)bits);
}

// Eight samples of T as a shift register of dwords: pop() takes the lowest sample, push() enters one at the top (after eight the group
// is in memory order).
template <typename T>
struct Group {
    static constexpr int B = 8 * sizeof(T), N = dp::kGroup * B / 32;
    uint32_t r[N];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < N; ++k) r[k] = 0;
    }
    __device__ __forceinline__ uint32_t pop() {
        if constexpr (B == 32) {  // a sample a dword: the registers move up whole
            const uint32_t s = r[0];
#pragma unroll
            for (int k = 0; k + 1 < N; ++k) r[k] = r[k + 1];
            return s;
        } else {
            const uint32_t s = r[0] & ((1u << B) - 1u);
#pragma unroll
            for (int k = 0; k + 1 < N; ++k) r[k] = (r[k] >> B) | (r[k + 1] << (32 - B));
            r[N - 1] >>= B;
            return s;
        }
    }
    __device__ __forceinline__ void push(uint32_t q) {
        static_assert(B < 32, "outputs are integers of 8 or 16 bits");
#pragma unroll
        for (int k = 0; k + 1 < N; ++k) r[k] = (r[k] >> B) | (r[k + 1] << (32 - B));
        r[N - 1] = (r[N - 1] >> B) | (q << (32 - B));
    }
    // samples [x0, x0 + 8) of a row, clipped to [0, w)
    __device__ __forceinline__ void load(const T *row, int x0, int w, bool vec) {
        if (vec && x0 + dp::kGroup <= w) {
            if constexpr (N == 2) {
                const u32x2 v = *reinterpret_cast<const u32x2 *>(row + x0);
                r[0] = v.x, r[1] = v.y;
            } else if constexpr (N == 4) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(row + x0);
                r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
            } else {  // 32-bit samples: two 16-byte loads
                const u32x4 a = *reinterpret_cast<const u32x4 *>(row + x0), b = *(reinterpret_cast<const u32x4 *>(row + x0) + 1);
                r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w, r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w;
            }
        } else {
            clear();
#pragma unroll
            for (int j = 0; j < dp::kGroup; ++j)
                if (x0 + j < w) r[j * B / 32] |= sample_bits(row[x0 + j]) << (j * B % 32);
        }
    }
    // the n samples pushed last to [x0, x0 + n) of a row
    __device__ __forceinline__ void store(T *row, int x0, int n, bool vec) {
        if (vec && n == dp::kGroup) {
            static_assert(N <= 4, "outputs are integers of 8 or 16 bits");
            if constexpr (N == 2) {
                u32x2 v;
                v.x = r[0], v.y = r[1];
                *reinterpret_cast<u32x2 *>(row + x0) = v;
            } else {
                u32x4 v;
                v.x = r[0], v.y = r[1], v.z = r[2], v.w = r[3];
                *reinterpret_cast<u32x4 *>(row + x0) = v;
            }
        } else {
            for (int k = n; k < dp::kGroup; ++k) push(0);
#pragma unroll
            for (int j = 0; j < dp::kGroup; ++j)
                if (j < n) row[x0 + j] = (T)(r[j * B / 32] >> (j * B % 32));
        }
    }
};

// lane i takes v of lane i - 1 (wave_shr:1), lane 0 takes `edge`
__device__ __forceinline__ float from_lane_above(float v, float edge) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

template <typename Tin, typename Tout, int WAVES>
__global__ __launch_bounds__(WAVES * dp::kLanes) void depth_diffuse_kernel(const DepthParams prm) {
    __shared__ float ringS[WAVES][dp::kRing];  // ringS[k]: the errors of wave k's last row, read by wave k + 1
    __shared__ float carryS[dp::kCarryLds];    // the last wave's last row, read by wave 0 in its next band
    const DepthPlane &f = prm.p[blockIdx.x];
    const int lane = threadIdx.x & (dp::kLanes - 1), k = __builtin_amdgcn_readfirstlane(threadIdx.x / dp::kLanes);
    const int w = f.w, h = f.h;
    const dp::Plan plan = dp::make_plan(w, h, WAVES);
    const bool carry_used = dp::has_carry(plan), carry_global = dp::carry_in_scratch(plan), svec = f.svec, dvec = f.dvec;
    float *const carryG = f.carry;
    const float scale = prm.scale, peak = prm.peak;

    // column c of the row above this wave's band: the ring of the wave above, or the carry row (an LDS read or a global one, never a
    // pointer chosen between the two: that would be a flat access)
    auto seam_read = [&](int c) -> float {
        if (k > 0) return ringS[k - 1][dp::ring_slot(c)];
        float v = carryS[c & (dp::kCarryLds - 1)];
        asm volatile("" : "+v"(v));  // keeps the two loads apart
        if (carry_global) v = carryG[c];
        return v;
    };

    float e = 0.0f, top_m1 = 0.0f, top_0 = 0.0f, top_p1 = 0.0f;  // the lane's last error; the row above at x - 1, x, x + 1
    Group<Tin> cur, next;
    Group<Tout> out;
    cur.clear(), next.clear(), out.clear();

    for (int g = 0; g < plan.chunks; ++g) {
        const dp::Slot sl = dp::slot_of(plan, k, g);
        if (sl.band >= 0) {
            const int y = sl.band * dp::kLanes + lane;
            const bool row_ok = y < h;
            const Tin *srow = static_cast<const Tin *>(f.src) + (size_t)(row_ok ? y : 0) * f.sstride;
            Tout *drow = static_cast<Tout *>(f.dst) + (size_t)(row_ok ? y : 0) * f.dstride;
            if (sl.step0 == 0) {  // a new band
                e = top_m1 = top_0 = top_p1 = 0.0f;
                if (row_ok) next.load(srow, 0, w, svec);
                // lane 0 starts at column 0: top[0] is not among the columns the steps bring (they begin with top[1])
                if (sl.band > 0 && lane == 0) top_p1 = seam_read(0);
            }
            // the chunk's seam columns, one a lane: what lane 0 receives at step step0 + i is the error of the row above at step0 + i + 1
            float seam = 0.0f;
            const int sc = dp::seam_column(sl.step0 + lane);
            if (sl.band > 0 && sc < w) seam = seam_read(sc);
            for (int i = 0; i < dp::kChunk; ++i) {
                const int x = dp::column_of(sl.step0 + i, lane);
                const float edge = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(seam), i));
                const float fresh = from_lane_above(e, edge);
                top_m1 = top_0, top_0 = top_p1, top_p1 = fresh;
                float en = 0.0f;  // a lane outside its row hands down 0: errors outside the plane are 0
                if (row_ok && x >= 0 && x < w) {
                    if ((x & (dp::kGroup - 1)) == 0) {
                        cur = next;
                        if (x + dp::kGroup < w) next.load(srow, x + dp::kGroup, w, svec);
                    }
                    const float q = dp::diffuse(sample_value<Tin>(cur.pop()), scale, peak, e, top_m1, top_0, top_p1, &en);
                    out.push((uint32_t)q);
                    if ((x & (dp::kGroup - 1)) == dp::kGroup - 1 || x == w - 1) out.store(drow, x & ~(dp::kGroup - 1), (x & (dp::kGroup - 1)) + 1, dvec);
                    if (lane == dp::kLanes - 1) {
                        if (k < WAVES - 1)
                            ringS[k][dp::ring_slot(x)] = en;
                        else if (carry_used) {
                            if (carry_global)
                                carryG[x] = en;
                            else
                                carryS[x] = en;
                        }
                    }
                }
                e = en;
            }
        }
        __syncthreads();
    }
}

template <typename Tin, typename Tout>
void launch_none(vszip_ctx *ctx, int blocks, const DepthParams &t) {
    hipLaunchKernelGGL((depth_none_kernel<Tin, Tout>), dim3(blocks), dim3(kRowUnitThreads), 0, ctx->stream, t);
}
template <typename Tin, typename Tout>
void launch_diffuse(vszip_ctx *ctx, int waves, int blocks, const DepthParams &t) {
    if (waves == dp::kWavesSmall)
        hipLaunchKernelGGL((depth_diffuse_kernel<Tin, Tout, dp::kWavesSmall>), dim3(blocks), dim3(dp::kWavesSmall * dp::kLanes), 0, ctx->stream, t);
    else
        hipLaunchKernelGGL((depth_diffuse_kernel<Tin, Tout, dp::kWavesLarge>), dim3(blocks), dim3(dp::kWavesLarge * dp::kLanes), 0, ctx->stream, t);
}
#endif  // __HIPCC__

bool aligned16(const void *p, ptrdiff_t stride, size_t size) { return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)((size_t)stride * size)) & 15) == 0; }

// one plane's entry
template <typename Tin, typename Tout>
void depth_fill(DepthPlane &d, const vszip_depth_plane &s, float *carry) {
    d.src = s.src;
    d.dst = s.dst;
    d.carry = carry;
    d.sstride = (int)s.src_stride;
    d.dstride = (int)s.dst_stride;
    d.w = s.w;
    d.h = s.h;
    d.svec = aligned16(s.src, s.src_stride, sizeof(Tin));
    d.dvec = aligned16(s.dst, s.dst_stride, sizeof(Tout));
    constexpr int V = (sizeof(Tin) == 1 || sizeof(Tout) == 1) ? 16 : 8;
    d.rows = (short)vszip_rows_per_workgroup(d.svec && d.dvec ? s.w / V : s.w);
}

// the planes `idx` of the table through one kernel: waves 0 none, else the error-diffusion workgroup
template <typename Tin, typename Tout>
int depth_run(vszip_ctx *ctx, const vszip_depth_plane *planes, const std::vector<int> &idx, int waves, DepthParams &prm,
              const std::vector<scratch::Region<float>> &carry, char *base) {
    return vszip_for_each_table(
        ctx, prm, (int)idx.size(),
        [&](DepthPlane &d, int j) -> int {
            const int i = idx[j];
            depth_fill<Tin, Tout>(d, planes[i], carry[i].count ? carry[i].in(base) : nullptr);
            return waves ? 1 : (planes[i].h + d.rows - 1) / d.rows;
        },
        [&](const DepthParams &t, int blocks, int) {
            vszip_probe_scope probe(ctx);
            if (waves)
                launch_diffuse<Tin, Tout>(ctx, waves, blocks, t);
            else
                launch_none<Tin, Tout>(ctx, blocks, t);
            return VSZIP_OK;
        });
}

}  // namespace

#ifndef VSZIP_DEPTH_KERNELS_ONLY  // depth_fmt.hip instantiates the kernels above for float sources; the entry points are built once, here
int vszip_depth_waves(const vszip_ctx *ctx, int h) {
    const int forced = ctx->opt.depth_waves;
    return forced == dp::kWavesSmall || forced == dp::kWavesLarge ? forced : dp::waves_for(h);
}

void vszip_depth_take_carry(const vszip_ctx *ctx, scratch::Layout &lay, const vszip_depth_plane *planes, int nplanes, int dither,
                            std::vector<scratch::Region<float>> &carry) {
    carry.assign(nplanes, scratch::Region<float>());
    if (!dither) return;
    for (int i = 0; i < nplanes; ++i)
        if (dp::carry_in_scratch(dp::make_plan(planes[i].w, planes[i].h, vszip_depth_waves(ctx, planes[i].h)))) carry[i] = lay.take<float>((size_t)planes[i].w, 256);
}

int vszip_depth_queue(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, int bits_in, int bits_out, int dither, int full_range,
                      const std::vector<scratch::Region<float>> &carry, char *base) {
    DepthParams prm;
    prm.scale = dp::scale_of(bits_in, bits_out, full_range != 0);
    prm.peak = (float)((1u << bits_out) - 1u);
    // none: every plane through one kernel; error diffusion: the planes of either workgroup size through theirs
    std::vector<int> idx[2];
    for (int i = 0; i < nplanes; ++i) idx[dither && vszip_depth_waves(ctx, planes[i].h) == dp::kWavesLarge].push_back(i);
    for (int c = 0; c < 2; ++c) {
        if (idx[c].empty()) continue;
        const int waves = !dither ? 0 : c ? dp::kWavesLarge : dp::kWavesSmall;
        int rc;
        if (bits_in == 8)
            rc = bits_out == 8 ? depth_run<uint8_t, uint8_t>(ctx, planes, idx[c], waves, prm, carry, base) : depth_run<uint8_t, uint16_t>(ctx, planes, idx[c], waves, prm, carry, base);
        else
            rc = bits_out == 8 ? depth_run<uint16_t, uint8_t>(ctx, planes, idx[c], waves, prm, carry, base) : depth_run<uint16_t, uint16_t>(ctx, planes, idx[c], waves, prm, carry, base);
        if (rc != VSZIP_OK) return rc;
    }
    return VSZIP_OK;
}

VSZIP_EXPORT int vszip_depth(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, int bits_in, int bits_out, int dither, int full_range) {
    if (!ctx) return VSZIP_ERR_ARG;
    char msg[256];
    const int bad = vszip_depth_check(bits_in, bits_out, dither, full_range, planes, nplanes, msg, sizeof msg);
    if (bad != VSZIP_OK) return vszip_set_error(ctx, bad, "%s", msg);
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    scratch::Layout lay;
    std::vector<scratch::Region<float>> carry;
    vszip_depth_take_carry(ctx, lay, planes, nplanes, dither, carry);
    char *base = nullptr;
    if (lay.bytes()) {
        const int rc = vszip_reserve_scratch(ctx, lay, &base);
        if (rc != VSZIP_OK) return rc;
    }
    return vszip_depth_queue(ctx, planes, nplanes, bits_in, bits_out, dither, full_range, carry, base);
}
#endif  // VSZIP_DEPTH_KERNELS_ONLY
