// Row bands of boxblur_ct_ring_kernel: how many bands a plane is cut into, and which rows each one owns.
// Plain C++ (no HIP): the launch code plans with it, the kernel decodes its band with band_y0(), and
// tests/ring_bands_check.cpp sweeps it on the host.
//
// A plane of h rows in nb bands gives band `by` the rows [by * h / nb, (by + 1) * h / nb): the bands tile
// the plane, their row counts differ by at most one, and no row is done twice. A band is never shorter
// than one ring period (nr rows): the kernel's prologue fills a whole ring, and the row queue's first
// requests, before it looks at the band's end.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace ring_bands {

// the constants of one kernel instance that the plan depends on
struct Consts {
    int nr;         // ring period in rows (RingGeom::NR)
    int halo_rows;  // rows a band reads that its neighbours read too (RingGeom::HALO_ROWS)
    int slots;      // wave slots of the chip for this instance: 256 CUs x 4 SIMDs x waves a SIMD
};

// planes of one height and tile count (a batch is a few geometries repeated: luma and chroma of every frame)
struct Geo {
    int h, ntx, count;
};

// first row of band `by` (by == nb: one past the plane's last row)
constexpr int band_y0(int by, int h, int nb) { return (int)((long long)by * h / nb); }

// bands of a plane of h rows when bands of about `target` ring periods are wanted
inline int bands_for(int h, int nr, int target) {
    const int periods = (h + nr - 1) / nr;
    return std::max(1, std::min(h / nr, (periods + target / 2) / target));
}

// The choice of `target` trades re-read halo rows (shorter bands = more traffic) against how well the
// waves fill the chip's wave slots over time: with W waves of up to max_len rows running in
// ceil(W / slots) generations, the fraction of slot-time doing work is
//     eff = total_work / (slots * generations * max_len),
// and measured launch times follow  total_work * (1 + 0.3 * (1 - eff))  within a few percent
// (64 4K frames, r = 13 — 4 + 2 bands, 3072 waves = every slot: 603 us; bands of 26 periods: 635 us;
// 16: 1.17 generations, 710 us; 39: half the slots, 694 us). Work is counted in rows a tile:
// rows + nb * halo_rows, the longest band is ceil(h / nb) + halo_rows.
inline double plan_cost(const std::vector<Geo> &geos, const Consts &c, int target, double *waves_out) {
    double work = 0, waves = 0, max_len = 0;
    for (const Geo &g : geos) {
        const int nb = bands_for(g.h, c.nr, target);
        const double ntx = (double)g.ntx * g.count;
        work += ntx * (g.h + nb * c.halo_rows);
        waves += ntx * nb;
        max_len = std::max(max_len, (double)((g.h + nb - 1) / nb + c.halo_rows));
    }
    *waves_out = waves;
    const double gens = std::ceil(waves / c.slots);
    const double eff = std::min(1.0, work / (c.slots * gens * max_len));
    // a launch that cannot fill the chip ends with its longest wave (a lone wave steps about
    // three times as fast as one of a full chip): small inputs get many short bands
    return std::max(work / c.slots * (1.0 + 0.3 * (1.0 - eff)), 0.3 * max_len);
}

// Band length of a launch, in ring periods (returned; *waves_ret = the waves of that plan).
// (small launches run out of the 256 MiB Infinity Cache and reward occupancy more than the
// model says: never go below 60 % of the slots when shorter bands can fill them)
inline int plan_target(const std::vector<Geo> &geos, const Consts &c, double *waves_ret) {
    double waves = 0;
    int target = 1;
    double best = plan_cost(geos, c, 1, &waves);
    double best_waves = waves;
    const double min_waves = std::min(0.6 * c.slots, waves);
    for (int t = 2; t <= 96; ++t) {
        const double cost = plan_cost(geos, c, t, &waves);
        if (waves >= min_waves && cost < best) {
            best = cost;
            best_waves = waves;
            target = t;
        }
    }
    *waves_ret = best_waves;
    return target;
}

}  // namespace ring_bands
