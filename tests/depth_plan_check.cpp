// Host check of the error-diffusion schedule (vapoursynth-zip_amd/csrc/depth_plan.hpp, plain C++): a stand-alone program, built by
// tests/test_depth_plan_host.py with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer. It replays the schedule as
// depth.hip's kernel walks it - chunk by chunk, wave by wave, step by step, lane by lane, with the same window of three errors, the same
// seam fetch at the start of a chunk and the same seam writes - for every workgroup size the kernel is built for, and checks that
//   * every sample of the plane is computed exactly once;
//   * every error a sample reads is the error of the sample the recurrence names ((y, x - 1), (y - 1, x - 1 .. x + 1), or 0 outside the
//     plane): within a wave it comes from the lane above one step earlier, across a seam it was written in a chunk before the chunk that
//     reads it (a barrier lies between) and the slot still holds it;
//   * no seam slot is written in a chunk in which another wave reads it, and none is overwritten before its last read (a read would
//     find another sample's error);
//   * every wave executes plan.chunks barriers and has nothing left to do after them;
//   * the recurrence run in that order gives the bits of the serial restatement.
// It also prints the size and field offsets of vszip_depth_plane as the C compiler lays it out (compared with the ctypes class).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/vszip_hip.h"
#include "depth_plan.hpp"

namespace dp = depth_plan;

static long failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);      \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

struct Err {  // an error value and whose it is (y < 0: the 0 of outside the plane)
    float v = 0.0f;
    int y = -1, x = 0;
};
struct SeamSlot {
    Err e;
    int written = -1, read = -1;  // the chunks of the last write and the last read
};

static uint32_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}

// the recurrence as the issue states it, row by row
static std::vector<uint16_t> serial(const std::vector<uint16_t> &src, int w, int h, float scale, float peak) {
    std::vector<uint16_t> out((size_t)w * h);
    std::vector<float> top(w + 2, 0.0f), cur(w + 2, 0.0f);
    for (int y = 0; y < h; ++y) {
        float left = 0.0f;
        for (int x = 0; x < w; ++x) {
            float e;
            out[(size_t)y * w + x] = (uint16_t)dp::diffuse((float)src[(size_t)y * w + x], scale, peak, left, top[x], top[x + 1], top[x + 2], &e);
            left = cur[x + 1] = e;
        }
        top = cur;
    }
    return out;
}

static bool is(const Err &e, int y, int x, int w, int h) {  // e is the error of (y, x), or the 0 of outside the plane
    if (y < 0 || y >= h || x < 0 || x >= w) return e.y < 0 && e.v == 0.0f;
    return e.y == y && e.x == x;
}

static long samples_swept = 0, plans_swept = 0;

static void sweep(int w, int h, int waves, int bits_in, int bits_out, uint64_t seed) {
    const dp::Plan plan = dp::make_plan(w, h, waves);
    const float scale = dp::scale_of(bits_in, bits_out, false), peak = (float)((1u << bits_out) - 1u);
    std::vector<uint16_t> src((size_t)w * h), got((size_t)w * h, 0xffff);
    std::vector<int> count((size_t)w * h, 0);
    for (size_t i = 0; i < src.size(); ++i) {
        const uint32_t r = splitmix(seed);
        // runs at 0 and at the peak so that the clamp feeds the error, noise elsewhere
        src[i] = (r >> 20) % 7 == 0 ? 0 : (r >> 20) % 7 == 1 ? (uint16_t)((1u << bits_in) - 1u) : (uint16_t)(r & ((1u << bits_in) - 1u));
    }
    std::vector<std::vector<SeamSlot>> ring(waves, std::vector<SeamSlot>(dp::kRing));
    std::vector<SeamSlot> carry(w);
    struct Lane {
        Err e, top_m1, top_0, top_p1;
    };
    std::vector<std::vector<Lane>> lanes(waves, std::vector<Lane>(dp::kLanes));
    std::vector<int> barriers(waves, 0);

    for (int g = 0; g < plan.chunks; ++g) {
        for (int k = 0; k < waves; ++k) {
            const dp::Slot sl = dp::slot_of(plan, k, g);
            ++barriers[k];
            if (sl.band < 0) continue;
            CHECK(sl.band % waves == k && dp::band_start_chunk(plan, sl.band) + sl.step0 / dp::kChunk == g, "w %d h %d waves %d: wave %d chunk %d band %d", w, h, waves, k, g, sl.band);
            std::vector<Lane> &L = lanes[k];
            auto fetch = [&](int c) {  // column c of the row above the band, through the seam
                SeamSlot &s = k > 0 ? ring[k - 1][dp::ring_slot(c)] : carry[c];
                CHECK(k > 0 || dp::has_carry(plan), "w %d h %d waves %d: a carry read without a carry row", w, h, waves);
                CHECK(s.written >= 0 && s.written < g, "w %d h %d waves %d: band %d reads column %d in chunk %d, written in chunk %d", w, h, waves, sl.band, c, g, s.written);
                CHECK(is(s.e, sl.band * dp::kLanes - 1, c, w, h), "w %d h %d waves %d: band %d column %d: the slot holds (%d, %d)", w, h, waves, sl.band, c, s.e.y, s.e.x);
                s.read = g;
                return s.e;
            };
            if (sl.step0 == 0) {
                for (Lane &l : L) l = Lane();
                if (sl.band > 0) L[0].top_p1 = fetch(0);  // lane 0 starts at column 0: top[0] is not among the columns the steps bring
            }
            // the seam fetch at the chunk's start, one column a lane
            Err seam[dp::kLanes];
            for (int j = 0; j < dp::kLanes; ++j) {
                const int c = dp::seam_column(sl.step0 + j);
                if (sl.band > 0 && c < w) seam[j] = fetch(c);
            }
            for (int i = 0; i < dp::kChunk; ++i) {
                std::vector<Err> before(dp::kLanes);
                for (int l = 0; l < dp::kLanes; ++l) before[l] = L[l].e;  // what the wave shift moves: every lane's error of the step before
                for (int l = 0; l < dp::kLanes; ++l) {
                    Lane &me = L[l];
                    const int y = sl.band * dp::kLanes + l, x = dp::column_of(sl.step0 + i, l);
                    me.top_m1 = me.top_0, me.top_0 = me.top_p1, me.top_p1 = l > 0 ? before[l - 1] : seam[i];
                    Err en;
                    if (y < h && x >= 0 && x < w) {
                        CHECK(is(me.e, y, x - 1, w, h) && is(me.top_m1, y - 1, x - 1, w, h) && is(me.top_0, y - 1, x, w, h) && is(me.top_p1, y - 1, x + 1, w, h),
                              "w %d h %d waves %d: sample (%d, %d) reads left (%d, %d) top (%d, %d) (%d, %d) (%d, %d)", w, h, waves, y, x, me.e.y, me.e.x, me.top_m1.y, me.top_m1.x,
                              me.top_0.y, me.top_0.x, me.top_p1.y, me.top_p1.x);
                        got[(size_t)y * w + x] = (uint16_t)dp::diffuse((float)src[(size_t)y * w + x], scale, peak, me.e.v, me.top_m1.v, me.top_0.v, me.top_p1.v, &en.v);
                        en.y = y, en.x = x;
                        ++count[(size_t)y * w + x];
                        if (l == dp::kLanes - 1 && (k < waves - 1 || dp::has_carry(plan))) {
                            SeamSlot &s = k < waves - 1 ? ring[k][dp::ring_slot(x)] : carry[x];
                            CHECK(s.read < g, "w %d h %d waves %d: band %d writes column %d in chunk %d, in which it is read", w, h, waves, sl.band, x, g);
                            // the slot's last value must have had its read, if it has a reader at all (the last band's does not)
                            if (s.written >= 0 && s.e.y + 1 < h) CHECK(s.read >= s.written, "w %d h %d waves %d: the error of (%d, %d) is overwritten unread", w, h, waves, s.e.y, s.e.x);
                            s.e = en, s.written = g;
                        }
                    }
                    me.e = en;
                }
            }
        }
    }
    for (int k = 0; k < waves; ++k) {
        CHECK(barriers[k] == plan.chunks, "w %d h %d waves %d: wave %d counts %d barriers of %d", w, h, waves, k, barriers[k], plan.chunks);
        for (int g = plan.chunks; g < plan.chunks + 2 * plan.sweep_chunks; ++g) CHECK(dp::slot_of(plan, k, g).band < 0, "w %d h %d waves %d: wave %d has work in chunk %d", w, h, waves, k, g);
    }
    long once = 0;
    for (int c : count) once += c == 1;
    CHECK(once == (long)w * h, "w %d h %d waves %d: %ld of %ld samples computed exactly once", w, h, waves, once, (long)w * h);
    const std::vector<uint16_t> want = serial(src, w, h, scale, peak);
    CHECK(std::memcmp(want.data(), got.data(), want.size() * sizeof(uint16_t)) == 0, "w %d h %d waves %d %d -> %d: the schedule's bits differ from the serial restatement's", w, h, waves,
          bits_in, bits_out);
    samples_swept += (long)w * h;
    ++plans_swept;
}

#define LAYOUT_BEGIN(T) printf("struct %s size %zu", #T, sizeof(T))
#define FIELD(T, f) printf(" %s %zu", #f, offsetof(T, f))

int main() {
    const int ws[] = {1, 2, 3, 63, 64, 65, 129, 300}, hs[] = {1, 2, 63, 64, 65, 129, 257, 1030}, waves[] = {dp::kWavesSmall, dp::kWavesLarge};
    const int depths[][2] = {{16, 8}, {16, 10}, {10, 8}, {16, 15}};
    uint64_t seed = 1;
    int d = 0;
    for (int nw : waves)
        for (int w : ws)
            for (int h : hs) sweep(w, h, nw, depths[d % 4][0], depths[d % 4][1], seed++), ++d;
    // rows wider than a wave's lag times the workgroup (the wave, not the band above, decides when a band starts), and a carry row that leaves LDS
    sweep(900, 300, dp::kWavesSmall, 16, 8, seed++);
    sweep(1283, 270, dp::kWavesSmall, 16, 8, seed++);
    // w = 256 m + 2: the row's last column shares its ring slot with column 1 of the wave's next band, which without the spare chunk of
    // sweep_chunks would be written in the very chunk that reads it
    sweep(770, 260, dp::kWavesSmall, 16, 8, seed++);
    sweep(1026, 520, dp::kWavesSmall, 16, 8, seed++);
    sweep(3100, 1030, dp::kWavesLarge, 16, 8, seed++);
    sweep(dp::kCarryLds + 3, 260, dp::kWavesSmall, 16, 8, seed++);
    CHECK(dp::carry_in_scratch(dp::make_plan(dp::kCarryLds + 3, 260, dp::kWavesSmall)) && !dp::carry_in_scratch(dp::make_plan(dp::kCarryLds, 260, dp::kWavesSmall)) &&
              !dp::carry_in_scratch(dp::make_plan(dp::kCarryLds + 3, 256, dp::kWavesSmall)),
          "where the carry row lives");
    CHECK(dp::waves_for(256) == dp::kWavesSmall && dp::waves_for(257) == dp::kWavesLarge, "the workgroup by rows");

    LAYOUT_BEGIN(vszip_depth_plane);
    FIELD(vszip_depth_plane, src);
    FIELD(vszip_depth_plane, src_stride);
    FIELD(vszip_depth_plane, dst);
    FIELD(vszip_depth_plane, dst_stride);
    FIELD(vszip_depth_plane, w);
    FIELD(vszip_depth_plane, h);
    FIELD(vszip_depth_plane, chroma);
    printf("\n");
    printf("%ld plans swept, %ld samples, %ld failures\n", plans_swept, samples_swept, failures);
    return failures ? 1 : 0;
}
