// Stand-alone host check of the BilateralDither point-list generator (vszip_bilateral_dither_points and _derive of
// vapoursynth-zip_amd/csrc/host_params.cpp), built together with that file under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_bilateral_dither_points_host.py. Sweeps radius 2 .. 48 with subspl 0, 4, 8, 16 and 4096; geometries with K >= 32 build a
// void-and-cluster matrix each, so only those named in kLarge run. Per geometry: K as derive gives it, 23 lists that start with (0, 0),
// no point twice within a list, every point inside the window; and one line "r subspl K checksum" that the Python side compares
// with the numpy spec's.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../include/vszip_hip.h"

static const int kLarge[][2] = {{7, 4}, {9, 8}, {10, 4}, {11, 4}, {12, 16}, {16, 4}, {16, 8}, {17, 0}, {24, 0}, {33, 16}, {40, 4}, {48, 4}};

int main() {
    int failures = 0, geometries = 0, large = 0;
    const float subs[] = {0.0f, 4.0f, 8.0f, 16.0f, 4096.0f};
    for (int r = 2; r <= 48; ++r)
        for (float s : subs) {
            int32_t K = 0;
            if (vszip_bilateral_dither_points(r, s, nullptr, 0, &K) != VSZIP_OK) {
                std::printf("FAIL query r=%d subspl=%g\n", r, (double)s);
                ++failures;
                continue;
            }
            vszip_bilateral_dither_cfg cfg;
            if (vszip_bilateral_dither_derive(0, 8, r, 2.5f, 0.4f, 0.0f, s, &cfg, nullptr, 0) != VSZIP_OK || cfg.K != K || !cfg.subsampled || K < 3 || K > 4096) {
                std::printf("FAIL derive r=%d subspl=%g K=%d\n", r, (double)s, K);
                ++failures;
                continue;
            }
            if (K >= 32) {
                bool listed = false;
                for (const auto &g : kLarge) listed |= g[0] == r && (float)g[1] == s;
                if (!listed) continue;
                ++large;
            }
            std::vector<int16_t> pts((size_t)23 * K * 2, (int16_t)0x7fff);  // exactly the capacity asked for: ASan watches the end
            if (vszip_bilateral_dither_points(r, s, pts.data(), (size_t)23 * K, &K) != VSZIP_OK) {
                std::printf("FAIL generate r=%d subspl=%g\n", r, (double)s);
                ++failures;
                continue;
            }
            bool ok = true;
            for (int l = 0; l < 23; ++l) {
                const int16_t *p = pts.data() + (size_t)l * K * 2;
                ok &= p[0] == 0 && p[1] == 0;
                std::set<std::pair<int, int>> seen;
                for (int k = 0; k < K; ++k) {
                    ok &= p[2 * k] > -r && p[2 * k] < r && p[2 * k + 1] > -r && p[2 * k + 1] < r;
                    ok &= seen.insert({p[2 * k], p[2 * k + 1]}).second;
                }
            }
            uint64_t sum = 0;
            for (size_t i = 0; i < pts.size(); ++i) sum += ((uint64_t)(uint16_t)pts[i] + 1) * ((uint64_t)i * 2654435761ull + 12345ull);
            std::printf("geometry %d %g %d %llu\n", r, (double)s, K, (unsigned long long)sum);
            if (!ok) {
                std::printf("FAIL lists r=%d subspl=%g K=%d\n", r, (double)s, K);
                ++failures;
            }
            ++geometries;
        }
    // a capacity one pair short is refused, nothing written
    int16_t two[4] = {1, 2, 3, 4};
    if (vszip_bilateral_dither_points(2, 4096.0f, two, 2, nullptr) != VSZIP_ERR_ARG || two[0] != 1) ++failures;
    std::printf("%d geometries, %d with K >= 32, %d failures\n", geometries, large, failures);
    return failures ? 1 : 0;
}
