// Host check of the BoxBlur ring kernel's band planner (vapoursynth-zip_amd/csrc/ring_bands.hpp), run by tests/test_ring_bands_host.py
// under AddressSanitizer + UndefinedBehaviorSanitizer. Sweeps plane heights, ring periods and band targets and checks what the kernel relies on:
// the bands tile the plane, none is shorter than a ring period, and their row counts differ by at most one.
#include <cstdio>
#include <vector>

#include "ring_bands.hpp"

static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (++failures <= 20) {               \
                std::printf("FAIL %s: ", #cond);  \
                std::printf(__VA_ARGS__);         \
                std::printf("\n");                \
            }                                     \
        }                                         \
    } while (0)

int main() {
    long plans = 0, bands = 0;
    for (int h = 53; h <= 2200; ++h)
        for (int nr = 4; nr <= 46; ++nr)
            for (int target = 1; target <= 96; ++target) {
                const int nb = ring_bands::bands_for(h, nr, target);
                CHECK(nb >= 1 && nb * nr <= h, "h=%d nr=%d target=%d nb=%d", h, nr, target, nb);
                if (nb < 1) continue;
                ++plans;
                CHECK(ring_bands::band_y0(0, h, nb) == 0 && ring_bands::band_y0(nb, h, nb) == h, "h=%d nb=%d: bands do not span the plane", h, nb);
                int shortest = h, longest = 0, covered = 0;
                for (int by = 0; by < nb; ++by) {
                    const int y0 = ring_bands::band_y0(by, h, nb), y1 = ring_bands::band_y0(by + 1, h, nb);
                    CHECK(y0 == covered, "h=%d nb=%d band %d starts at %d, the one before ended at %d", h, nb, by, y0, covered);  // no gap, no overlap
                    CHECK(y1 - y0 >= nr, "h=%d nr=%d nb=%d band %d has %d rows", h, nr, nb, by, y1 - y0);
                    shortest = std::min(shortest, y1 - y0);
                    longest = std::max(longest, y1 - y0);
                    covered = y1;
                    ++bands;
                }
                CHECK(covered == h, "h=%d nb=%d: rows up to %d", h, nb, covered);
                CHECK(longest - shortest <= 1, "h=%d nb=%d: bands of %d .. %d rows", h, nb, shortest, longest);
                CHECK(longest == (h + nb - 1) / nb, "h=%d nb=%d: longest band %d rows, the cost model counts %d", h, nb, longest, (h + nb - 1) / nb);
            }

    // the headline batch: 64 4K YUV420P16 frames at r = 13 (ring period 28, 26 halo rows, three waves a SIMD)
    {
        const std::vector<ring_bands::Geo> geos = {{2160, 8, 64}, {1080, 4, 64}, {1080, 4, 64}};
        const ring_bands::Consts c = {28, 26, 3072};
        double waves = 0;
        const int target = ring_bands::plan_target(geos, c, &waves);
        long n = 0;
        for (const ring_bands::Geo &g : geos) {
            const int nb = ring_bands::bands_for(g.h, c.nr, target);
            CHECK(nb == g.h / 540, "headline: %d bands for %d rows (target %d)", nb, g.h, target);
            for (int by = 0; by < nb; ++by) {
                const int rows = ring_bands::band_y0(by + 1, g.h, nb) - ring_bands::band_y0(by, g.h, nb);
                CHECK(rows == 540, "headline: h=%d band %d has %d rows", g.h, by, rows);
            }
            n += (long)nb * g.ntx * g.count;
        }
        CHECK(n == 3072 && waves == 3072.0, "headline: %ld bands, planner says %.0f waves", n, waves);
        std::printf("headline: target %d periods, %ld bands of 540 rows\n", target, n);
    }
    std::printf("%ld plans, %ld bands, %d failures\n", plans, bands, failures);
    return failures ? 1 : 0;
}
