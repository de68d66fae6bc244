// The schedule of the error-diffusion kernel of depth.hip, in plain C++: which lane makes which sample at which step, where the errors
// that cross a wave's band travel, how far a wave runs behind the one above it and how many barriers a workgroup executes. The kernel
// and tests/depth_plan_check.cpp (which replays the schedule on the host and checks every hand-over) read the same functions.
//
// A sample (y, x) needs the errors of (y, x - 1) and of (y - 1, x - 1 .. x + 1). One workgroup of `waves` waves owns one plane. The
// plane's rows are cut into bands of 64; band b belongs to wave b % waves, lane l of it to row 64 b + l. Time runs in steps; a band
// that starts at step t_b has lane l at column (t - t_b) - 2 l at step t, so the lane above is always two columns ahead and its
// freshest error (column x + 1, made one step ago) arrives by a wave shift. Row 64 b - 1 belongs to another wave: its errors go through
// LDS. Steps come in chunks of kChunk, a barrier after each; band b starts kLagChunks chunks after band b - 1, which is enough for
// everything lane 0 reads during a chunk (it reads it all at the chunk's start, one column a lane) to have been written before the
// previous barrier. A wave's next band (b + waves) starts when the wave is free and the band above it is kLagChunks ahead, whichever is
// later: sweep_chunks is the period of that.
//
// Seams. Between wave k - 1 and wave k (k >= 1) a ring of kRing columns: the distance between writer and reader is fixed. Between the
// last wave and wave 0 the distance grows with the plane's width (the wave has to finish its band first), so that seam is a whole row
// of errors, the carry row: in LDS up to kCarryLds columns, in the context's scratch beyond.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define DEPTH_PLAN_HD __host__ __device__ __forceinline__
#else
#define DEPTH_PLAN_HD inline
#endif

namespace depth_plan {

constexpr int kLanes = 64;                           // rows of a band
constexpr int kSkew = 2;                             // columns a lane runs behind the lane above
constexpr int kChunk = 64;                           // steps between two barriers
constexpr int kDrain = kSkew * (kLanes - 1);         // steps lane 63 runs behind lane 0
constexpr int kLagChunks = kDrain / kChunk + 2;      // chunks a band starts behind the band above
constexpr int kRing = 256;                           // columns of a seam ring
constexpr int kCarryLds = 4096;                      // widest carry row kept in LDS
constexpr int kGroup = 8;                            // samples a lane loads / stores at once
constexpr int kWavesSmall = 4, kWavesLarge = 16;     // the workgroup sizes the kernel is built for
constexpr int kSmallRows = kWavesSmall * kLanes;     // planes up to this many rows take the small workgroup

static_assert(kChunk == kLanes, "a chunk's seam columns are fetched one a lane");
static_assert(kWavesSmall >= 2, "a wave never reads the seam it writes");

struct Plan {
    int w, h, waves;
    int bands;         // ceil(h / 64)
    int band_chunks;   // chunks a band takes: w + kDrain steps
    int sweep_chunks;  // chunks between a wave's bands
    int chunks;        // chunks (= barriers) of the whole plane, the same for every wave
};

DEPTH_PLAN_HD int waves_for(int h) { return h <= kSmallRows ? kWavesSmall : kWavesLarge; }

DEPTH_PLAN_HD Plan make_plan(int w, int h, int waves) {
    Plan p;
    p.w = w;
    p.h = h;
    p.waves = waves;
    p.bands = (h + kLanes - 1) / kLanes;
    p.band_chunks = (w + kDrain + kChunk - 1) / kChunk;
    // (+ 1: lane 63 of a wave's next band writes ring slots from its second chunk on, and the wave below reads the band before for
    // kLagChunks chunks longer; with the extra chunk every slot's last read lies before the barrier that precedes its next write)
    p.sweep_chunks = p.band_chunks + 1 > waves * kLagChunks ? p.band_chunks + 1 : waves * kLagChunks;
    p.chunks = ((p.bands - 1) / waves) * p.sweep_chunks + ((p.bands - 1) % waves) * kLagChunks + p.band_chunks;  // the last band's start + its length
    return p;
}

// the chunk band b starts in
DEPTH_PLAN_HD int band_start_chunk(const Plan &p, int b) { return (b / p.waves) * p.sweep_chunks + (b % p.waves) * kLagChunks; }

// What wave k does in chunk g: the band it is in (-1: it idles to the barrier) and the first step of the chunk, counted from the band's start.
struct Slot {
    int band, step0;
};
DEPTH_PLAN_HD Slot slot_of(const Plan &p, int k, int g) {
    const int rel = g - k * kLagChunks;
    if (rel < 0) return {-1, 0};
    const int sweep = rel / p.sweep_chunks, lc = rel - sweep * p.sweep_chunks, b = sweep * p.waves + k;
    if (lc >= p.band_chunks || b >= p.bands) return {-1, 0};
    return {b, lc * kChunk};
}

DEPTH_PLAN_HD int column_of(int step, int lane) { return step - kSkew * lane; }  // may be outside [0, w): the lane idles
// the column of the row above whose error a lane receives at `step` (made by the lane above one step earlier): top[x + 1]
DEPTH_PLAN_HD int seam_column(int step) { return step + 1; }
DEPTH_PLAN_HD int ring_slot(int column) { return column & (kRing - 1); }
// does the plane need a carry row, and does it leave LDS
DEPTH_PLAN_HD bool has_carry(const Plan &p) { return p.bands > p.waves; }
DEPTH_PLAN_HD bool carry_in_scratch(const Plan &p) { return has_carry(p) && p.w > kCarryLds; }

// ---- the arithmetic (IEEE f32, every operation rounded on its own: built with contraction off) ---------------------------------
// scale of a conversion; full-range chroma (a non-zero offset) is not served
inline float scale_of(int bits_in, int bits_out, bool full_range) {
    if (!full_range) return bits_out >= bits_in ? (float)(1u << (bits_out - bits_in)) : 1.0f / (float)(1u << (bits_in - bits_out));
    return (float)((double)((1u << bits_out) - 1u) / (double)((1u << bits_in) - 1u));
}
// dither none
DEPTH_PLAN_HD float convert_none(float src, float scale, float peak) { return rintf(fminf(fmaxf(src * scale, 0.0f), peak)); }
// one sample of the error diffusion: the quantised value; *err_out its error. top_m1 / top_0 / top_p1: the errors of the row above at x - 1, x, x + 1
DEPTH_PLAN_HD float diffuse(float src, float scale, float peak, float left, float top_m1, float top_0, float top_p1, float *err_out) {
    const float x0 = src * scale;
    float err = 0.0f + left * (7.0f / 16.0f);
    err = err + top_p1 * (3.0f / 16.0f);
    err = err + top_0 * (5.0f / 16.0f);
    err = err + top_m1 * (1.0f / 16.0f);
    const float v = fminf(fmaxf(x0 + err, 0.0f), peak);
    const float q = rintf(v);
    *err_out = v - q;
    return q;
}

}  // namespace depth_plan
