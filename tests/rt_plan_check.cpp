// Host check of the RT BoxBlur's schedule planner (vapoursynth-zip_amd/csrc/rt_plan.hpp), run by tests/test_rt_plan_host.py under
// AddressSanitizer + UndefinedBehaviorSanitizer. (1) Sweeps sample types, plane sets, radii, pass counts, alignment and the shipped option
// combinations and checks what the executor (boxblur_rt.hip, run_rt) and the kernels rely on. (2) Compares the planner with the recorded launch
// schedules (tests/rt_schedules.json, recorded on the GPU with tools/rt_schedule_calls.py; the test passes them as the text file argv[1]):
// a change of routing fails here and has to re-record the file on purpose.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rt_plan.hpp"

using rt_plan::Kind;
using rt_plan::Plane;
using rt_plan::Step;

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

struct Type {
    const char *name;
    rt_plan::Elem e;
};
static const Type kTypes[] = {{"u8", {true, 1}}, {"u16", {true, 2}}, {"f16", {false, 2}}, {"f32", {false, 4}}};
constexpr int kPlanesPerLaunch = 192;  // plane_table.hpp: planes of one kernel launch (a step launches once per table)

static bool is_chain(Kind k) { return k == Kind::FloatChain || k == Kind::IntChainWhole || k == Kind::IntChainBanded; }

// what run_rt and the kernels rely on, for one plan
static void check_plan(const std::vector<Step> &plan, const std::vector<Plane> &pl, const rt_plan::Elem &e, int hr, int hp, int vr, int vp, const char *what) {
    const int nh = hr > 0 && hp > 0 ? hp : 0, nv = vr > 0 && vp > 0 ? vp : 0;
    int hsum = 0, vsum = 0, maxh = 0;
    for (const Plane &q : pl) maxh = std::max(maxh, q.h);
    bool seen_vertical = false;
    CHECK((int)plan.size() <= nh + nv, "%s: %zu steps for %d passes", what, plan.size(), nh + nv);
    for (size_t k = 0; k < plan.size(); ++k) {
        const Step &s = plan[k];
        CHECK(s.span >= 1, "%s step %zu: span %d", what, k, s.span);
        (s.vertical ? vsum : hsum) += s.span;
        if (s.vertical) seen_vertical = true;
        CHECK(s.vertical || !seen_vertical, "%s step %zu: a horizontal step after a vertical one", what, k);
        CHECK(s.radius == (s.vertical ? vr : hr), "%s step %zu: radius %d", what, k, s.radius);
        // exactly the last step writes the caller's planes; a step reads what the step before wrote, never the scratch set it writes
        CHECK(s.to_dst == (k + 1 == plan.size()), "%s step %zu of %zu: to_dst %d", what, k, plan.size(), (int)s.to_dst);
        CHECK(s.to_dst ? s.scratch == -1 : (s.scratch == 0 || s.scratch == 1), "%s step %zu: scratch %d", what, k, s.scratch);
        if (k > 0) CHECK(plan[k - 1].scratch != s.scratch, "%s step %zu reads scratch set %d and writes it", what, k, s.scratch);
        if (e.is_int)
            CHECK(s.kind != Kind::FloatChain && (s.vertical ? s.kind != Kind::HSmall : (s.kind == Kind::Pass || s.kind == Kind::HSmall)), "%s step %zu: kind %d on an integer plan", what, k, (int)s.kind);
        else
            CHECK(s.kind == Kind::Pass || s.kind == Kind::FloatChain, "%s step %zu: kind %d on a float plan", what, k, (int)s.kind);
        if (s.kind == Kind::Pass) CHECK(s.span == 1, "%s step %zu: a pass of span %d", what, k, s.span);
        if (s.kind == Kind::HSmall) CHECK(s.span == hp && k == 0 && s.radius <= rt_plan::kHsMaxR, "%s step %zu: hsmall span %d radius %d", what, k, s.span, s.radius);
        if (is_chain(s.kind)) {
            CHECK(s.span >= 2 && s.span <= rt_plan::kFcMaxPass, "%s step %zu: chain of %d", what, k, s.span);
            const size_t lds = rt_plan::chain_lds_bytes(e, s.radius, s.span, s.vertical);
            CHECK(lds <= (size_t)(s.vertical ? 48 : 30) * 1024, "%s step %zu: %zu bytes of LDS", what, k, lds);
        }
        CHECK((s.band_rows > 0) == (s.kind == Kind::IntChainBanded), "%s step %zu: kind %d with band_rows %d", what, k, (int)s.kind, s.band_rows);
        if (s.kind == Kind::IntChainBanded) CHECK((maxh + s.band_rows - 1) / s.band_rows >= 2, "%s step %zu: bands of %d rows on %d rows", what, k, s.band_rows, maxh);
    }
    CHECK(hsum == nh && vsum == nv, "%s: spans sum to %d + %d, passes %d + %d", what, hsum, vsum, nh, nv);
}

static Plane caller_plane(int h, int w, const rt_plan::Elem &e, bool aligned) {
    const int stride = aligned ? (w + 31) & ~31 : w + 1;
    const unsigned low = aligned ? 0u : (unsigned)((e.sample_bytes | stride * e.sample_bytes) & 15);  // (misaligned: pointers offset by one sample)
    return Plane{w, h, stride, stride, low, low};
}

static long sweep() {
    const int dims[] = {3, 5, 20, 35, 64, 70, 131, 540, 1080, 2160};
    const int radii[] = {1, 2, 5, 8, 13, 16, 17, 22, 30, 127, 128};
    struct OptSet {
        const char *name;
        rt_plan::Opts o;
    };
    std::vector<OptSet> optsets(6);
    optsets[0].name = "default";
    optsets[1].name = "ICHAIN_ALL", optsets[1].o.rt_ichain_all = 1;
    optsets[2].name = "NO_ICHAIN+NO_HSMALL", optsets[2].o.rt_no_ichain = 1, optsets[2].o.rt_no_hsmall = 1;
    optsets[3].name = "NO_BANDED", optsets[3].o.rt_no_banded = 1;
    optsets[4].name = "FCHAIN_ALL", optsets[4].o.rt_fchain_all = 1;
    optsets[5].name = "NO_FCHAIN", optsets[5].o.rt_no_fchain = 1;
    // plane sets as (h, w) lists: every single plane, pairs and 4:2:0 triples along the diagonal, and batches large enough for the gates on waves and rows
    std::vector<std::vector<std::pair<int, int>>> sets;
    for (int h : dims)
        for (int w : dims) sets.push_back({{h, w}});
    for (int i = 0; i < 10; ++i) sets.push_back({{dims[i], dims[9 - i]}, {dims[(i + 3) % 10], dims[(i + 7) % 10]}});
    for (int i = 2; i < 10; ++i) sets.push_back({{dims[i], dims[(i + 1) % 10]}, {dims[i] / 2, dims[(i + 1) % 10] / 2}, {dims[i] / 2, dims[(i + 1) % 10] / 2}});
    for (int frames : {8, 64}) {
        std::vector<std::pair<int, int>> b;
        for (int f = 0; f < frames; ++f) b.insert(b.end(), {{1080, 1920}, {540, 960}, {540, 960}});
        sets.push_back(b);
    }
    long plans = 0;
    char what[256];
    for (const Type &t : kTypes)
        for (const auto &set : sets)
            for (int aligned = 1; aligned >= 0; --aligned) {
                std::vector<Plane> pl;
                int minw = 1 << 30, minh = 1 << 30;
                for (const auto &hw : set) {
                    pl.push_back(caller_plane(hw.first, hw.second, t.e, aligned != 0));
                    minh = std::min(minh, hw.first);
                    minw = std::min(minw, hw.second);
                }
                for (int r : radii)
                    for (int hp = 0; hp <= 7; ++hp)
                        for (int vp = 0; vp <= 7; ++vp) {
                            if (hp + vp == 0) continue;
                            if ((hp > 0 && 2 * r >= minw) || (vp > 0 && 2 * r >= minh)) continue;  // (vszip_boxblur refuses these)
                            for (const OptSet &os : optsets) {
                                std::snprintf(what, sizeof what, "%s %zu planes first %dx%d %s r=%d passes %d+%d %s", t.name, set.size(), set[0].second, set[0].first, aligned ? "aligned" : "offset", r, hp, vp, os.name);
                                check_plan(rt_plan::rt_plan(pl.data(), (int)pl.size(), t.e, os.o, r, hp, r, vp), pl, t.e, r, hp, r, vp, what);
                                ++plans;
                            }
                        }
            }
    return plans;
}

// ---- the recorded schedules --------------------------------------------------------------------------------------------------------------------
struct Launch {
    std::string name;
    long grid, wg, lds;
};
struct Call {
    std::string label;
    const Type *type = nullptr;
    int frames = 0, hr = 0, hp = 0, vr = 0, vp = 0;
    std::vector<Plane> base;
    rt_plan::Opts opts;
    std::vector<Launch> launches;
};

static bool starts_with(const std::string &s, const char *p) { return s.compare(0, std::strlen(p), p) == 0; }
// the per-pass kernels by axis (the row / column kernel of a Pass step is chosen per table: only the axis is compared)
static bool is_hpass(const std::string &n) {
    return starts_with(n, "boxblur_rt_hring_kernel<") || starts_with(n, "boxblur_rt_hrow_kernel<") || starts_with(n, "boxblur_rt_hint_kernel<") || starts_with(n, "boxblur_rt_float_h_kernel<") ||
           starts_with(n, "boxblur_ct_ring_kernel<") || starts_with(n, "boxblur_ct_int_kernel<");
}
static bool is_vpass(const std::string &n) { return starts_with(n, "boxblur_rt_vband_kernel<") || starts_with(n, "boxblur_rt_vint_kernel<") || starts_with(n, "boxblur_rt_float_v_kernel<"); }

static bool set_option(rt_plan::Opts &o, const char *name, int v) {
    struct {
        const char *name;
        int rt_plan::Opts::*field;
    } const map[] = {{"VSZIP_RT_NO_HSMALL", &rt_plan::Opts::rt_no_hsmall}, {"VSZIP_RT_NO_ICHAIN", &rt_plan::Opts::rt_no_ichain}, {"VSZIP_RT_NO_FCHAIN", &rt_plan::Opts::rt_no_fchain},
                     {"VSZIP_RT_ICHAIN_ALL", &rt_plan::Opts::rt_ichain_all}, {"VSZIP_RT_FCHAIN_ALL", &rt_plan::Opts::rt_fchain_all}, {"VSZIP_RT_NO_BANDED", &rt_plan::Opts::rt_no_banded}};
    for (const auto &m : map)
        if (!std::strcmp(m.name, name)) {
            o.*m.field = v;
            return true;
        }
    return false;
}

// Lines: "call <type> <frames> <hr> <hp> <vr> <vp> <label>", "plane <h> <w> <sstride> <dstride> <src_low> <dst_low>", "opt <NAME> <value>",
// "k <grid threads> <workgroup> <lds bytes> <kernel name>"
static std::vector<Call> read_calls(const char *path) {
    std::vector<Call> calls;
    std::FILE *f = std::fopen(path, "r");
    if (!f) return calls;
    char line[1024], a[64], rest[900];
    while (std::fgets(line, sizeof line, f)) {
        int v[6];
        long g, wg, lds;
        if (std::sscanf(line, "call %63s %d %d %d %d %d %899[^\n]", a, &v[0], &v[1], &v[2], &v[3], &v[4], rest) == 7) {
            Call c;
            for (const Type &t : kTypes)
                if (!std::strcmp(t.name, a)) c.type = &t;
            c.frames = v[0], c.hr = v[1], c.hp = v[2], c.vr = v[3], c.vp = v[4], c.label = rest;
            CHECK(c.type, "unknown type %s", a);
            if (c.type) calls.push_back(c);
        } else if (!calls.empty() && std::sscanf(line, "plane %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
            calls.back().base.push_back(Plane{v[1], v[0], v[2], v[3], (unsigned)v[4], (unsigned)v[5]});
        } else if (!calls.empty() && std::sscanf(line, "opt %63s %d", a, &v[0]) == 2) {
            CHECK(set_option(calls.back().opts, a, v[0]), "unknown option %s", a);
        } else if (!calls.empty() && std::sscanf(line, "k %ld %ld %ld %899[^\n]", &g, &wg, &lds, rest) == 4) {
            calls.back().launches.push_back(Launch{rest, g, wg, lds});
        } else {
            CHECK(line[0] == '\n' || line[0] == '#', "unreadable line: %s", line);
        }
    }
    std::fclose(f);
    return calls;
}

static long check_recorded(const char *path) {
    const std::vector<Call> calls = read_calls(path);
    long launches = 0;
    char what[300], name[128];
    for (const Call &c : calls) {
        std::vector<Plane> pl;
        for (int fr = 0; fr < c.frames; ++fr) pl.insert(pl.end(), c.base.begin(), c.base.end());
        std::snprintf(what, sizeof what, "recorded '%s' %s x%d (%d,%d,%d,%d)", c.label.c_str(), c.type->name, c.frames, c.hr, c.hp, c.vr, c.vp);
        const rt_plan::Elem &e = c.type->e;
        const std::vector<Step> plan = rt_plan::rt_plan(pl.data(), (int)pl.size(), e, c.opts, c.hr, c.hp, c.vr, c.vp);
        check_plan(plan, pl, e, c.hr, c.hp, c.vr, c.vp, what);
        const int ntab = ((int)pl.size() + kPlanesPerLaunch - 1) / kPlanesPerLaunch;
        size_t at = 0;  // next recorded launch
        auto expect = [&](const char *kname, long blocks, size_t lds) {
            if (at >= c.launches.size()) {
                CHECK(false, "%s: the plan launches %s, the record has ended", what, kname);
                return;
            }
            const Launch &l = c.launches[at++];
            CHECK(l.name == kname && l.grid == blocks * 64 && l.wg == 64 && l.lds == (long)lds, "%s launch %zu: planned %s grid %ld lds %zu, recorded %s grid %ld wg %ld lds %ld", what, at - 1, kname,
                  blocks * 64, lds, l.name.c_str(), l.grid, l.wg, l.lds);
        };
        for (size_t k = 0; k < plan.size(); ++k) {
            const Step &s = plan[k];
            if (s.kind == Kind::Pass) {
                // this and the Pass steps of the same axis that follow it: at least one launch each, of that axis's per-pass kernels, and nothing else
                size_t k1 = k;
                while (k1 + 1 < plan.size() && plan[k1 + 1].kind == Kind::Pass && plan[k1 + 1].vertical == s.vertical) ++k1;
                size_t n = 0;
                while (at < c.launches.size() && (s.vertical ? is_vpass(c.launches[at].name) : is_hpass(c.launches[at].name))) ++at, ++n;
                CHECK(n >= k1 - k + 1, "%s: %zu %s Pass steps, %zu launches of per-pass kernels", what, k1 - k + 1, s.vertical ? "vertical" : "horizontal", n);
                k = k1;
                continue;
            }
            for (int t = 0; t < ntab; ++t) {
                const int p0 = t * kPlanesPerLaunch, p1 = std::min((int)pl.size(), p0 + kPlanesPerLaunch);
                long cols = 0, rows = 0, rowgroups = 0, bandwaves = 0;
                for (int i = p0; i < p1; ++i) {
                    cols += (pl[i].w + 63) / 64;
                    rows += pl[i].h;
                    rowgroups += (pl[i].h + rt_plan::kFcRB - 1) / rt_plan::kFcRB;
                    if (s.band_rows) bandwaves += (long)((pl[i].w + 63) / 64) * ((pl[i].h + s.band_rows - 1) / s.band_rows);
                }
                // (the recorded LDS bytes are a kernel's static LDS: the rings and rows that a launch adds dynamically are not in the trace; check_plan bounds them)
                switch (s.kind) {
                    case Kind::FloatChain:
                    case Kind::IntChainWhole:
                        std::snprintf(name, sizeof name, "boxblur_rt_float_%cchain_kernel<%s, %d>", s.vertical ? 'v' : 'h', c.type->name, s.span);
                        expect(name, s.vertical ? cols : rowgroups, s.vertical ? 0 : 2 * rt_plan::kFcRB * 65 * sizeof(float));  // (the horizontal kernel's two [kFcRB][65] f32 tiles)
                        break;
                    case Kind::IntChainBanded:
                        std::snprintf(name, sizeof name, "boxblur_rt_ichain_kernel<%s, %d, 1>", c.type->name, s.span);
                        expect(name, cols, 0);
                        std::snprintf(name, sizeof name, "boxblur_rt_ichain_kernel<%s, %d, 2>", c.type->name, s.span);
                        expect(name, bandwaves, 0);
                        break;
                    case Kind::HSmall:
                        std::snprintf(name, sizeof name, "boxblur_rt_hsmall_kernel<%s, %d>", c.type->name, s.radius);
                        expect(name, rows, 0);
                        break;
                    default: CHECK(false, "%s step %zu: kind %d is not in a default build", what, k, (int)s.kind);
                }
            }
        }
        CHECK(at == c.launches.size(), "%s: %zu launches recorded, the plan accounts for %zu", what, c.launches.size(), at);
        launches += (long)c.launches.size();
    }
    std::printf("%zu recorded calls, %ld launches\n", calls.size(), launches);
    return (long)calls.size();
}

int main(int argc, char **argv) {
    const long plans = sweep();
    if (argc > 1) check_recorded(argv[1]);
    std::printf("%ld plans, %d failures\n", plans, failures);
    return failures ? 1 : 0;
}
