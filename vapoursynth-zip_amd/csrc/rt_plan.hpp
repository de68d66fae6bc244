// The pass schedule of the RT BoxBlur (boxblur_rt.hip): which of hpasses horizontal and vpasses vertical passes share a launch, which kernel
// family takes each launch, and where its output goes. Plain C++ (no HIP, no vszip_ctx): run_rt plans with it and then only executes the steps;
// the kernels take their geometry constants from here; tests/rt_plan_check.cpp sweeps it on the host and compares it with the kernel sequences
// recorded in tests/rt_schedules.json, so a change of routing fails a CPU test.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

namespace rt_plan {

// ---- what the kernels and the predicates share -------------------------------------------------------------------------------------------
constexpr int kFcMaxPass = 5;  // the chain kernels: 2 ... 5 passes, lines of at least 2 R + 2 samples, rings within one workgroup's LDS
constexpr int kFcPf = 32;      // vertical chain: rows of one register set (three rotate; [kFcPf][64] parked rows in LDS)
constexpr int kFcRB = 64;      // horizontal chain: rows a wave
constexpr int kHsMaxR = 16, kHsMaxW = 8192, kHsHalo = 16;  // boxblur_rt_hsmall_kernel (radius 13 x 5 passes is the reference README's third benchmark)
constexpr int kVsMaxR = 8;     // boxblur_rt_vsmall_kernel (a development variant)

// One plane as a step sees it. The planner is given the caller's planes; a step's source is the caller's source (first step) or the step
// before's destination, its destination the caller's destination (last step) or a scratch plane. Scratch planes are 16-byte aligned with a
// pitch of (w + 63) & ~63 samples.
struct Plane {
    int w, h;
    int sstride, dstride;       // pitches in samples
    unsigned src_low, dst_low;  // the low four bits of pointer | pitch in bytes: all that alignment tests look at
};
struct Elem {
    bool is_int;
    int sample_bytes;
};
// the fields of vszip_options (options.inc) that the decisions read
struct Opts {
    int rt_no_hsmall = 0, rt_no_ichain = 0, rt_no_fchain = 0, rt_ichain_all = 0, rt_fchain_all = 0;
    int rt_no_banded = 0, rt_ichain_bands = 0;
    int rt_vsmall = 0, rt_vsmall_max = 2, rt_no_vsmall = 0;
};

enum class Kind {
    Pass,            // launch_pass: one pass, the row / column kernel chosen per table
    FloatChain,      // launch_fchain on float planes: boxblur_rt_float_hchain / vchain_kernel<T, span>
    IntChainWhole,   // launch_fchain on integer planes: boxblur_rt_float_vchain_kernel<T, span>, a wave per 64 whole columns
    IntChainBanded,  // launch_ichain_banded: boxblur_rt_ichain_kernel<T, span, 1 | 2>, bands of band_rows rows
    HSmall,          // launch_hsmall: boxblur_rt_hsmall_kernel<T, radius>, every horizontal pass
    VSmall,          // launch_vsmall: boxblur_rt_vsmall_kernel<T, span> (a development variant)
};
struct Step {
    Kind kind;
    bool vertical;
    int radius, span;  // span passes of this radius along the axis
    int band_rows;     // 0 unless IntChainBanded
    bool to_dst;       // writes the caller's planes (the last step), else ...
    int scratch;       // ... this one of the two scratch plane sets (-1 with to_dst)
};

inline int scratch_pitch(int w) { return (w + 63) & ~63; }
// source, destination and both pitches (in bytes) are multiples of mask + 1 (mask <= 15)
inline bool aligned(const Plane &q, unsigned mask = 15) { return ((q.src_low | q.dst_low) & mask) == 0; }
// dynamic LDS of a chain launch: the stages' rings ([2R + 3][span] lines of a wave's 64 samples) and, vertical, kFcPf parked rows + 8 output rows
inline size_t chain_lds_bytes(const Elem &e, int radius, int npass, bool vertical) {
    const size_t esz = e.is_int ? sizeof(uint16_t) : sizeof(float);  // FcArith<T>::E: what a ring holds
    return vertical ? ((size_t)npass * (2 * radius + 3) + kFcPf + 8) * 64 * esz : (size_t)npass * (2 * radius + 3) * kFcRB * sizeof(float);
}

// ---- who qualifies ------------------------------------------------------------------------------------------------------------------------
// all horizontal passes of a small radius in one launch (boxblur_rt_hsmall_kernel); false: the planes do not qualify
inline bool hsmall_ok(const Elem &e, const Opts &o, const std::vector<Plane> &pl, int radius, int npass) {
    if (!e.is_int || e.sample_bytes > 2 || npass < 2 || radius < 1 || radius > kHsMaxR || o.rt_no_hsmall) return false;
    for (const Plane &q : pl) {
        if (!aligned(q) || q.w <= 2 * radius || q.w > kHsMaxW || q.sstride < ((q.w + 7) / 8) * 8 || q.dstride < ((q.w + 7) / 8) * 8) return false;
    }
    return true;
}

// all vertical passes of a small radius in one launch (boxblur_rt_vsmall_kernel); false: the planes do not qualify
inline bool vsmall_ok(const Elem &e, const Opts &o, const std::vector<Plane> &pl, int radius, int npass) {
    // Measured (tools/boxblur_radii_probe.py, 1080p, 64 frames per call, against one launch per pass): two passes 93.3 k -> 107.7 k fps (u16), 105 k -> 108 k
    // (u8); three passes 68 k -> 66.5 k (u16), 79 k -> 65 k (u8) — the chain's rings and registers leave 6 waves a CU at three stages. Hence two passes
    // only (VSZIP_RT_VSMALL_MAX=3 / 4 for experiments).
    // End of round 3: OPT-IN (VSZIP_RT_VSMALL=1, a development variant: a default build has it off for good). The per-pass kernel's LDS ring with its software
    // pipeline (later that round) overtook it: two vertical passes, 1080p, 64 / 16 / 4 frames per call, two launches against this kernel: u8 r = 1 179 k / 191 k / 60 k fps
    // against 156 k / 160 k / 48 k, u16 147 k / 167 k / 68 k against 153 k / 160 k / 49 k; from r = 3 on this kernel falls to 64 - 105 k (its rings leave few waves a CU)
    // where two launches stay at 137 - 180 k (tools/boxblur_radii_probe.py).
    if (!o.rt_vsmall) return false;
    const int max_pass = std::min(4, std::max(2, o.rt_vsmall_max));
    if (!e.is_int || e.sample_bytes > 2 || npass < 2 || npass > max_pass || radius < 1 || radius > kVsMaxR || o.rt_no_vsmall) return false;
    if ((size_t)npass * (2 * radius + 2) * 1024 > 40 * 1024) return false;  // the rings: four waves a CU at least
    for (const Plane &q : pl) {
        if (!aligned(q) || q.h <= 2 * npass * radius + 2 || q.sstride < ((q.w + 7) / 8) * 8 || q.dstride < ((q.w + 7) / 8) * 8) return false;
    }
    return true;
}

// the chain kernels (float: either axis; integer: vertical, whole columns, or with bands >= 2 in bands of rows)
inline bool fchain_ok(const Elem &e, const Opts &o, const std::vector<Plane> &pl, int radius, int npass, bool vertical, int bands = 1) {
    const bool is_int = e.is_int;
    if ((is_int ? o.rt_no_ichain : o.rt_no_fchain) || npass < 2 || npass > kFcMaxPass) return false;
    if (is_int && (!vertical || e.sample_bytes > 2 || radius > 127)) return false;  // integer planes: the vertical chain only (the horizontal passes have boxblur_rt_hsmall_kernel)
    // 8-bit planes: the per-pass kernel moves 16 samples a lane and wins up to four passes and at larger radii (1080p, 64 frames per call, chain against a launch per pass:
    // r = 2 x 3 passes -11 %, 13 x 2 -19 %, 2 x 4 even, 3 x 5 +16 %; 16-bit planes: +12 ... +55 % throughout — tools/boxblur_radii_probe.py). VSZIP_RT_ICHAIN_ALL=1: every case (tests).
    if (is_int && bands < 2 && e.sample_bytes == 1 && !(npass >= 5 && radius <= 8) && !o.rt_ichain_all) return false;
    if (is_int && bands < 2 && !o.rt_ichain_all) {
        // Two passes: two launches of the per-pass kernel are as fast (u16, r >= 3: the chain +3 ... 8 % at 64 frames) and do not mind small calls. And the chain is as slow as its
        // longest column (a wave per 64 columns, ~0.1 us a tick): with fewer waves than SIMDs — a plugin context submits ONE frame per call — the per-pass kernels, which
        // cut a plane into bands, are several times faster (4 1080p frames, three passes: ~110 us against 3 x 25 us).
        if (npass < 3) return false;
        long waves = 0;
        for (const Plane &q : pl) waves += (q.w + 63) / 64;
        if (waves < 900) return false;
    }
    if (!is_int && !vertical && !o.rt_fchain_all) {
        // The horizontal chain carries 64 rows a wave and costs what a row's ticks cost however few waves there are; the per-pass kernel (16 rows a wave) is faster on small calls:
        // 4K YUV420PS, 3 passes of r = 5, 1 / 2 / 4 frames per call: chain 2.5 k / 5.0 k / 9.7 k fps, a launch per pass 3.0 k / 5.7 k / 9.2 k. (The vertical chain wins from one frame on.)
        long rows = 0;
        for (const Plane &q : pl) rows += q.h;
        if (rows < 12000) return false;
    }
    if (chain_lds_bytes(e, radius, npass, vertical) > (size_t)(vertical ? 48 : 30) * 1024) return false;  // (the horizontal kernel also holds two 64 x 64 tiles)
    for (const Plane &q : pl) {
        if ((vertical ? q.h : q.w) < 2 * radius + 2) return false;
        if (vertical) {  // rows go four samples a lane
            if (!aligned(q, 4 * (unsigned)e.sample_bytes - 1) || q.sstride < ((q.w + 3) & ~3) || q.w < 4) return false;
        }
    }
    return true;
}

// The banded integer vertical chain (boxblur_rt_ichain_kernel): the planes qualify when the unbanded chain does, are tall enough for the mirror
// extension (P (R + 1) + 1 rows) and for at least two bands of 2 P (2R + 1) rows — below that a band's warm-up is more than its rows.
// How many bands: a cost model fitted to tools/rt_band_sweep.py (profiles/r04_rt_band_sweep.txt: 12 workloads x 8 band counts). A wave's time is its ticks — the band's rows
// + P (2R + 1) warm-up + P (R + 1) drain — times the tick's latency, which grows with the waves sharing a SIMD (about +36 % per extra wave: LDS hand-overs and the
// loop-carried sums leave gaps that a second wave fills only partly); the rings' LDS bounds the resident waves (five stages of r = 13: 23.7 KB a wave, six waves a CU),
// beyond which waves queue. T(nb) = max(longest wave, all wave-ticks / resident waves) x slow(waves per SIMD); the band count with the smallest T wins, 1 = no bands
// (the planner then chooses between the whole-column chain and a launch per pass). Returns the rows of a band, 0: no bands.
inline int ichain_band_rows(const Elem &e, const Opts &o, const std::vector<Plane> &pl, int radius, int npass) {
    if (!e.is_int || e.sample_bytes > 2 || o.rt_no_banded) return 0;
    int maxh = 0, minh = 1 << 30;
    for (const Plane &q : pl) {
        maxh = std::max(maxh, q.h);
        minh = std::min(minh, q.h);
    }
    if (minh < npass * (radius + 1) + 1) return 0;  // (the mirror extension reflects once)
    if (o.rt_ichain_bands > 0) {  // (tests and sweeps: any band count)
        const int nb = std::min(o.rt_ichain_bands, std::max(1, maxh / 8));
        return nb < 2 ? 0 : (maxh + nb - 1) / nb;
    }
    const int warm = npass * (2 * radius + 1), drain = npass * (radius + 1);
    const size_t lds = chain_lds_bytes(e, radius, npass, true);
    const double cap = 256.0 * std::min<double>(16.0, std::floor(160.0 * 1024 / (double)lds));
    // A batch is a few geometries repeated (luma and chroma of every frame): the model is summed per geometry. Every term below is a whole number far
    // below 2^53, so the sums are exactly what a loop over every band of every plane gives — that loop was 40 us of the 43 us that planning a 64-frame
    // call took, and the whole plan is made before the first launch.
    struct Geo {
        int ncg, h, count;
    };
    std::vector<Geo> geos;
    for (const Plane &q : pl) {
        const int ncg = (q.w + 63) / 64;
        auto g = std::find_if(geos.begin(), geos.end(), [&](const Geo &x) { return x.ncg == ncg && x.h == q.h; });
        if (g == geos.end())
            geos.push_back(Geo{ncg, q.h, 1});
        else
            ++g->count;
    }
    auto cost = [&](int nb) {
        const int br = (maxh + nb - 1) / nb;
        double total = 0, waves = 0, longest = 0;
        for (const Geo &g : geos) {
            const double n = (double)g.count * g.ncg;  // column groups of this geometry: a wave each per band
            if (nb == 1) {  // whole columns: the generic ticks at both ends cost about three fast ones
                const double t = g.h + drain + 2.0 * warm;
                total += n * t;
                waves += n;
                longest = std::max(longest, t);
                continue;
            }
            // the plane's bands: nbp - 1 of br rows and the last one with the rest
            const int nbp = (g.h + br - 1) / br;
            const double t_full = br + warm + drain, t_last = g.h - (nbp - 1) * br + warm + drain;
            total += n * ((nbp - 1) * t_full + t_last);
            longest = std::max(longest, nbp > 1 ? t_full : t_last);
            waves += n * nbp;
        }
        // (a grid search over the five constants against the sweep's 12 x 9 measurements: the model's pick is the measured optimum on nine workloads and
        // within 4 % of it on the other three — profiles/r04_rt_band_sweep.txt, tools/rt_band_fit.py)
        const double conc = std::min(waves, cap), w = conc / 1024.0;
        const double slow = 1.0 + 0.2 * std::max(0.0, w - 0.75);
        double t = std::max(longest, total / conc) * slow;
        if (waves > conc) t += 0.3 * longest * slow;  // queued waves: the last ones run beside idle slots
        return t + (nb > 1 ? 1.0 * drain : 0.0);      // (+ the launch that fills the table of constants)
    };
    int best_nb = 1;
    double best = cost(1);
    for (int nb : {2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32}) {
        if ((maxh + nb - 1) / nb < 32) break;
        const double c = cost(nb);
        if (c < best) {
            best = c;
            best_nb = nb;
        }
    }
    return best_nb < 2 ? 0 : (maxh + best_nb - 1) / best_nb;
}

// ---- how many of the remaining passes of an axis the next step tries to take ----------------------------------------------------------------
// float: what is left of this axis's passes in chains of up to kFcMaxPass stages (6 = 3 + 3 rather than 5 + 1: a lone pass is a launch of its own)
inline int float_span(int rem) {
    if (rem < 2) return 1;
    return rem <= kFcMaxPass ? rem : (rem - kFcMaxPass == 1 ? kFcMaxPass - 1 : kFcMaxPass);
}
// integer, horizontal: every horizontal pass of a small radius at once (round 3), tried at the first pass only
inline int int_hspan(int p, int hpasses) { return p == 0 && hpasses >= 2 ? hpasses : 1; }
// integer, vertical: what is left of the vertical passes, in chains of nearly equal length. A chain of P stages costs every row band P (3 R + 2) rows of
// warm-up and drain and P (2 R + 3) ring rows of LDS, so short planes take shorter chains and pay another trip through memory instead:
// at most a quarter of the shortest plane's rows may be warm-up (r = 13 on 1080p 4:2:0, 540-row chroma: 5 passes as 3 + 2 - 292 us
// against 343 for one chain of 5 on 32 frames, 4 as 2 + 2 - 218 against 234; 4K keeps its chain of 5: 246 against 289;
// tools/rt_pass_scaling.py)
inline int int_vspan(int rem, int minh, int vradius) {
    if (rem < 2) return 1;
    const int pmax = std::max(2, std::min(kFcMaxPass, minh / (4 * (3 * vradius + 2))));
    const int nchains = (rem + pmax - 1) / pmax;
    return (rem + nchains - 1) / nchains;
}

// ---- the schedule ---------------------------------------------------------------------------------------------------------------------------
// boxblur.zig:85-112: hpasses horizontal passes, then vpasses vertical passes, over one group of planes that goes through all of them together.
// The order in which a span of several passes is offered:
//   float planes         the chain, else one pass
//   integer, vertical    vsmall (when it takes the planes, neither chain is asked), the chain in bands, the chain over whole columns, else one pass
//   integer, horizontal  hsmall, else one pass
// A span that nobody takes becomes ONE pass into scratch (it is not the last), and the next step computes a fresh span from what is left.
inline std::vector<Step> rt_plan(const Plane *planes, int nplanes, const Elem &e, const Opts &o, int hradius, int hpasses, int vradius, int vpasses) {
    const bool hb = hradius > 0 && hpasses > 0, vb = vradius > 0 && vpasses > 0;
    const int nh = hb ? hpasses : 0, total = nh + (vb ? vpasses : 0);
    std::vector<Step> steps;
    steps.reserve((size_t)std::max(total, 0));
    std::vector<Plane> cur(planes, planes + nplanes);
    auto point = [&](bool to_dst) {
        for (int i = 0; i < nplanes; ++i) {
            cur[i].dstride = to_dst ? planes[i].dstride : scratch_pitch(planes[i].w);
            cur[i].dst_low = to_dst ? planes[i].dst_low : 0u;
        }
    };
    int which = 0;
    for (int p = 0; p < total;) {
        const bool vertical = p >= nh;
        const int radius = vertical ? vradius : hradius;
        int span;
        if (!e.is_int) {
            span = float_span(vertical ? total - p : hpasses - p);
        } else if (vertical) {
            int minh = 1 << 30;
            for (const Plane &q : cur) minh = std::min(minh, q.h);
            span = int_vspan(total - p, minh, vradius);
        } else {
            span = int_hspan(p, hpasses);
        }
        point(p + span == total);
        Kind kind = Kind::Pass;
        int band_rows = 0;
        if (span > 1 && !e.is_int) {
            if (fchain_ok(e, o, cur, radius, span, vertical)) kind = Kind::FloatChain;
        } else if (span > 1 && vertical) {
            if (vsmall_ok(e, o, cur, vradius, span)) {
                kind = Kind::VSmall;
            } else {
                // integer planes: the chain in bands of rows (exact under any segmentation: see boxblur_rt_ichain_kernel) — a span of several passes means
                // total > 1, so the scratch that holds the bands' table of constants exists — else over whole columns (one column a lane, the stages' rings in LDS)
                const int br = ichain_band_rows(e, o, cur, vradius, span);
                if (br > 0 && fchain_ok(e, o, cur, vradius, span, true, (cur[0].h + br - 1) / br)) {
                    kind = Kind::IntChainBanded;
                    band_rows = br;
                } else if (fchain_ok(e, o, cur, vradius, span, true)) {
                    kind = Kind::IntChainWhole;
                }
            }
        } else if (span > 1) {
            if (hsmall_ok(e, o, cur, hradius, hpasses)) kind = Kind::HSmall;
        }
        if (kind == Kind::Pass && span > 1) {  // (the planes do not qualify: back to one pass per launch; this one is not the last)
            span = 1;
            point(false);
        }
        const bool to_dst = p + span == total;
        steps.push_back(Step{kind, vertical, radius, span, band_rows, to_dst, to_dst ? -1 : which});
        for (Plane &q : cur) {
            q.sstride = q.dstride;
            q.src_low = q.dst_low;
        }
        which ^= 1;
        p += span;
    }
    return steps;
}

}  // namespace rt_plan
