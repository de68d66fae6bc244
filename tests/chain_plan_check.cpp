// Host check of vapoursynth-zip_amd/csrc/chain_plan.hpp, the plan behind vszip_chain_ops (tests/test_chain_plan_host.py builds this with the host
// compiler under AddressSanitizer + UndefinedBehaviorSanitizer and runs it; no GPU, no HIP). It sweeps chains of 1 - 6 ops of every kind over tables of
// 1 - 3 plane slots and 1 - 5 frames in shuffled order, random process masks, the sample sizes 1 / 2 / 4, and checks on every plan what the header of
// include/vszip_hip.h promises: only the last writer of an entry writes the caller's dst; every op reads where the op before left the entry; no op reads
// memory that it, or another entry of the same op, writes (the neighbouring frames of the temporal ops included); the halves lie inside the reserved
// size and the regions of different entries do not overlap; entries no op writes are copies; neighbour entries are the clamped frame arithmetic. Then
// every malformed chain the header lists is refused, with the op index in the text. Last, it prints the size and the field offsets of every struct of
// vszip_chain_ops for the ctypes classes to be compared with.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../include/vszip_hip.h"
#include "chain_plan.hpp"

namespace cp = chain_plan;

static int failures = 0;
static long checks = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        ++checks;                                \
        if (!(cond)) {                           \
            if (++failures <= 20) {              \
                printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
                printf(__VA_ARGS__);             \
                printf("\n");                    \
            }                                    \
        }                                        \
    } while (0)

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    int range(int lo, int hi) { return lo + below(hi - lo + 1); }
};

// the sample types of every kind, written down a second time from the header's rule 4 (not taken from chain_plan.hpp)
static bool takes(int kind, int dtype) {
    const bool u8 = dtype == VSZIP_U8, u16 = dtype == VSZIP_U16, f16 = dtype == VSZIP_F16, f32 = dtype == VSZIP_F32, u32 = dtype == VSZIP_U32;
    switch (kind) {
        case VSZIP_STAGE_BOXBLUR: case VSZIP_STAGE_BILATERAL: return u8 || u16 || f16 || f32;
        case VSZIP_STAGE_LIMITER: return u8 || u16 || f16 || f32 || u32;
        case VSZIP_STAGE_CLAHE: return u8 || u16;
        case VSZIP_STAGE_COMB_MASK: case VSZIP_STAGE_COMB_MASK_MT: case VSZIP_STAGE_CHECKMATE: case VSZIP_STAGE_COMPRESS: return u8;
        case VSZIP_STAGE_DEBAND: return u16 || f32;
        case VSZIP_STAGE_MOSQUITO_NR: case VSZIP_STAGE_BILATERAL_DITHER: return u8 || u16 || f32;
    }
    return false;
}

struct Interval {  // memory as the plan names it: a caller's src or dst plane of an entry, or bytes of the chain buffer
    int where, entry;
    size_t lo, hi;
};
static Interval interval_of(const cp::Plan &p, const std::vector<cp::Entry> &e, int entry, int where) {
    if (where == cp::kSrc || where == cp::kDst) return {where, entry, 0, 0};
    const size_t lo = p.half_offset(entry, where, e.data());
    return {where, entry, lo, lo + p.half_bytes(entry, e.data())};
}
static bool overlap(const Interval &a, const Interval &b) {
    const bool abuf = a.where == cp::kHalf0 || a.where == cp::kHalf1, bbuf = b.where == cp::kHalf0 || b.where == cp::kHalf1;
    if (abuf != bbuf) return false;                          // the chain buffer is the context's own memory
    if (abuf) return a.lo < b.hi && b.lo < a.hi;
    return a.where == b.where && a.entry == b.entry;         // caller planes: a src is never written, dst planes overlap no src (the caller's part of the contract)
}

static int find_entry(const std::vector<cp::Entry> &e, int slot, long frame) {
    for (size_t i = 0; i < e.size(); ++i)
        if (e[i].slot == slot && e[i].frame == frame) return (int)i;
    return -1;
}

static void check_plan(const cp::Plan &p, int bps, const std::vector<cp::Op> &ops, const std::vector<cp::Entry> &e, const char *tag) {
    const int n = (int)e.size(), nops = (int)ops.size();
    CHECK(p.ok, "%s: %s", tag, p.why.c_str());
    if (!p.ok) return;
    CHECK((int)p.writers.size() == n && (int)p.offset.size() == n && (int)p.pitch.size() == n && (int)p.ops.size() == nops, "%s: sizes", tag);
    // writers, layout
    size_t end = 0;
    std::vector<int> copies;
    for (int i = 0; i < n; ++i) {
        int w = 0;
        for (const cp::Op &o : ops) w += o.process[e[i].slot] ? 1 : 0;
        CHECK(p.writers[i] == w, "%s: entry %d has %d writers, plan says %d", tag, i, w, p.writers[i]);
        CHECK(p.pitch[i] % 256 == 0 && p.pitch[i] >= (size_t)e[i].w * bps && p.pitch[i] < (size_t)e[i].w * bps + 256, "%s: entry %d pitch %zu", tag, i, p.pitch[i]);
        CHECK(p.offset[i] == end, "%s: entry %d starts at %zu, the entries before end at %zu (regions are dense and disjoint)", tag, i, p.offset[i], end);
        end = p.offset[i] + (w > 1 ? 2 * p.pitch[i] * (size_t)e[i].h : 0);
        if (w == 0) copies.push_back(i);
    }
    CHECK(p.bytes == end, "%s: %zu bytes reserved, regions end at %zu", tag, p.bytes, end);
    CHECK(p.copies == copies, "%s: the copies are the entries nothing writes", tag);
    // fmin .. fmax of every slot
    long fmin[3] = {0, 0, 0}, fmax[3] = {0, 0, 0};
    bool seen[3] = {false, false, false};
    for (const cp::Entry &x : e) {
        fmin[x.slot] = seen[x.slot] ? std::min<long>(fmin[x.slot], x.frame) : x.frame;
        fmax[x.slot] = seen[x.slot] ? std::max<long>(fmax[x.slot], x.frame) : x.frame;
        seen[x.slot] = true;
    }
    std::vector<int> cur(n, cp::kSrc), written(n, 0);
    for (int s = 0; s < nops; ++s) {
        const std::vector<cp::Step> &steps = p.ops[s];
        // the steps are the processed entries, in table order
        size_t k = 0;
        for (int i = 0; i < n; ++i)
            if (ops[s].process[e[i].slot]) {
                CHECK(k < steps.size() && steps[k].entry == i, "%s: op %d step %zu is not entry %d", tag, s, k, i);
                ++k;
            }
        CHECK(k == steps.size(), "%s: op %d has %zu steps, %zu entries to process", tag, s, steps.size(), k);
        if (k != steps.size()) return;
        std::vector<Interval> reads, writes;
        for (const cp::Step &st : steps) {
            const int i = st.entry;
            CHECK(st.reads == cur[i], "%s: op %d reads entry %d at %d, it was left at %d", tag, s, i, st.reads, cur[i]);
            const bool last = written[i] + 1 == p.writers[i];
            CHECK((st.writes == cp::kDst) == last, "%s: op %d entry %d: writes %d, last writer %d", tag, s, i, st.writes, (int)last);
            CHECK(st.writes == cp::kDst || st.writes == cp::kHalf0 || st.writes == cp::kHalf1, "%s: op %d entry %d writes %d", tag, s, i, st.writes);
            CHECK(st.writes == cp::kDst || p.writers[i] > 1, "%s: op %d entry %d writes a half it has no region for", tag, s, i);
            reads.push_back(interval_of(p, e, i, st.reads));
            writes.push_back(interval_of(p, e, i, st.writes));
            if (st.writes != cp::kDst) CHECK(writes.back().hi <= p.bytes && writes.back().lo >= p.offset[i] && writes.back().hi <= p.offset[i] + p.region_bytes(i, e.data()), "%s: op %d entry %d writes outside its region", tag, s, i);
            if (ops[s].temporal) {
                const int got[4] = {st.p2, st.p1, st.n1, st.n2};
                const int d[4] = {-2, -1, 1, 2};
                for (int j = 0; j < 4; ++j) {
                    const long f = std::min(std::max((long)e[i].frame + d[j], fmin[e[i].slot]), fmax[e[i].slot]);
                    const int want = find_entry(e, e[i].slot, f);
                    CHECK(got[j] == want && want >= 0, "%s: op %d entry %d (frame %d) neighbour %+d is entry %d, expected %d (frame %ld)", tag, s, i, e[i].frame, d[j], got[j], want, f);
                    if (got[j] >= 0 && got[j] < n) {
                        CHECK(cur[got[j]] == st.reads || ops[s].process[e[got[j]].slot], "%s: neighbour not in step with its entry", tag);
                        reads.push_back(interval_of(p, e, got[j], st.reads));  // read where the op before left THAT entry: same writer count, same place
                    }
                }
            } else {
                CHECK(st.p2 == -1 && st.p1 == -1 && st.n1 == -1 && st.n2 == -1, "%s: op %d is not temporal and has neighbours", tag, s);
            }
        }
        // a temporal op's neighbours are entries of the same slot, which this op processes too: they are all still where the op before left them
        if (ops[s].temporal)
            for (const cp::Step &st : steps)
                for (int nb : {st.p2, st.p1, st.n1, st.n2})
                    if (nb >= 0 && nb < n) CHECK(cur[nb] == st.reads && e[nb].slot == e[st.entry].slot, "%s: op %d entry %d: neighbour %d lies at %d, read at %d", tag, s, st.entry, nb, cur[nb], st.reads);
        for (const Interval &r : reads)
            for (const Interval &w : writes) CHECK(!overlap(r, w), "%s: op %d reads (%d, entry %d) what it writes (%d, entry %d)", tag, s, r.where, r.entry, w.where, w.entry);
        for (size_t a = 0; a < writes.size(); ++a)
            for (size_t b = a + 1; b < writes.size(); ++b) CHECK(!overlap(writes[a], writes[b]), "%s: op %d writes entries %d and %d to the same memory", tag, s, writes[a].entry, writes[b].entry);
        for (const cp::Step &st : steps) {
            cur[st.entry] = st.writes;
            ++written[st.entry];
        }
    }
    for (int i = 0; i < n; ++i) CHECK(p.writers[i] == 0 ? cur[i] == cp::kSrc : cur[i] == cp::kDst, "%s: entry %d ends at %d", tag, i, cur[i]);
}

static std::vector<cp::Entry> clip_table(Rng &r, int slots, int frames, bool shuffle) {
    std::vector<cp::Entry> e;
    const int first = r.range(-3, 1000);
    int w[3], h[3];
    for (int k = 0; k < 3; ++k) w[k] = r.range(3, 700), h[k] = r.range(5, 300);
    for (int f = 0; f < frames; ++f)
        for (int k = 0; k < slots; ++k) {
            cp::Entry x;
            x.slot = k, x.frame = first + f, x.w = w[k], x.h = h[k];
            e.push_back(x);
        }
    if (shuffle)
        for (size_t i = e.size(); i > 1; --i) std::swap(e[i - 1], e[(size_t)r.below((int)i)]);
    return e;
}

static void sweep() {
    Rng r{2024};
    const int dtypes[3] = {VSZIP_U8, VSZIP_U16, VSZIP_F32};
    long plans = 0, temporal_plans = 0, kinds_seen[cp::kKinds] = {0};
    for (int nops = 1; nops <= 6; ++nops)
        for (int slots = 1; slots <= 3; ++slots)
            for (int frames = 1; frames <= 5; ++frames)
                for (int di = 0; di < 3; ++di)
                    for (int rep = 0; rep < 40; ++rep) {
                        const int dtype = dtypes[di], bps = cp::sample_bytes(dtype);
                        std::vector<cp::Op> ops(nops);
                        bool temporal = false;
                        for (cp::Op &o : ops) {
                            do o.kind = r.below(cp::kKinds);
                            while (!takes(o.kind, dtype));
                            for (int k = 0; k < 3; ++k) o.process[k] = r.below(3) != 0;
                            o.temporal = o.kind == VSZIP_STAGE_CHECKMATE || (o.kind == VSZIP_STAGE_COMB_MASK && r.below(2));
                            temporal = temporal || o.temporal;
                            ++kinds_seen[o.kind];
                        }
                        const std::vector<cp::Entry> e = clip_table(r, slots, frames, rep % 4 != 0);
                        const int bits = dtype == VSZIP_U8 ? 8 : dtype == VSZIP_U16 ? r.range(9, 16) : r.below(33);
                        char tag[96];
                        snprintf(tag, sizeof tag, "ops %d slots %d frames %d bytes %d rep %d", nops, slots, frames, bps, rep);
                        check_plan(cp::make(dtype, bits, ops.data(), nops, e.data(), (int)e.size(), true), bps, ops, e, tag);
                        ++plans;
                        temporal_plans += temporal;
                        if (!temporal) {  // without a temporal op the table is any table: no frame numbers, frames twice, sizes mixed
                            std::vector<cp::Entry> any = e;
                            for (cp::Entry &x : any) x.frame = r.below(2), x.w = r.range(1, 300), x.h = r.range(1, 90);
                            check_plan(cp::make(dtype, bits, ops.data(), nops, any.data(), (int)any.size(), rep % 2 == 0), bps, ops, any, tag);
                        }
                    }
    printf("%ld plans swept, %ld with a temporal op\n", plans, temporal_plans);
    for (int k = 0; k < cp::kKinds; ++k) CHECK(kinds_seen[k] > 100, "kind %d occurred %ld times", k, kinds_seen[k]);
    CHECK(temporal_plans > 1000, "temporal plans: %ld", temporal_plans);
}

static cp::Op op_of(int kind, bool temporal = false) {
    cp::Op o;
    o.kind = kind;
    o.process[0] = o.process[1] = o.process[2] = true;
    o.temporal = temporal;
    return o;
}
static void refused(const cp::Plan &p, const char *what, const char *needle, int bad_op) {
    CHECK(!p.ok, "%s is accepted", what);
    CHECK(p.why.find(needle) != std::string::npos, "%s: the text '%s' does not say '%s'", what, p.why.c_str(), needle);
    CHECK(p.bad_op == bad_op, "%s: names op %d, not %d", what, p.bad_op, bad_op);
    CHECK(p.ops.empty() && p.bytes == 0, "%s: a refused plan schedules nothing", what);
}

static void refusals() {
    Rng r{7};
    const std::vector<cp::Entry> clip = clip_table(r, 3, 4, true);
    const int n = (int)clip.size();
    const cp::Op blur = op_of(VSZIP_STAGE_BOXBLUR), cm = op_of(VSZIP_STAGE_CHECKMATE, true), comb = op_of(VSZIP_STAGE_COMB_MASK, true), still = op_of(VSZIP_STAGE_COMB_MASK, false);
    const cp::Op ops[3] = {blur, cm, comb};
    CHECK(cp::make(VSZIP_U8, 8, ops, 3, clip.data(), n, true).ok, "the well-formed clip is refused");
    // the frame table
    for (int which = 1; which <= 2; ++which) {
        char need[16];
        snprintf(need, sizeof need, "op %d ", which);
        const cp::Op two[3] = {blur, which == 1 ? cm : blur, which == 2 ? comb : blur};
        std::vector<cp::Entry> t = clip;
        int last = t[0].frame;
        for (const cp::Entry &x : t) last = std::max(last, x.frame);
        for (cp::Entry &x : t)
            if (x.frame == last && x.slot == 1) x.frame += 7;
        refused(cp::make(VSZIP_U8, 8, two, 3, t.data(), n, true), "a gap in the frames of a slot", "gap", which);
        CHECK(cp::make(VSZIP_U8, 8, two, 3, t.data(), n, true).why.find(need) != std::string::npos, "the text names op %d", which);
        t = clip;
        int a = -1;
        for (int i = 0; i < n && a < 0; ++i)
            for (int j = i + 1; j < n; ++j)
                if (t[i].slot == t[j].slot) { t[j].frame = t[i].frame; a = j; break; }
        refused(cp::make(VSZIP_U8, 8, two, 3, t.data(), n, true), "a (slot, frame) pair twice", "", which);
        t = clip;
        t[(size_t)r.below(n)].w += 1;
        refused(cp::make(VSZIP_U8, 8, two, 3, t.data(), n, true), "mixed sizes in a slot", "differs in size", which);
        t = clip;
        t[(size_t)r.below(n)].h += 2;
        refused(cp::make(VSZIP_U8, 8, two, 3, t.data(), n, true), "mixed heights in a slot", "differs in size", which);
        refused(cp::make(VSZIP_U8, 8, two, 3, clip.data(), n, false), "NULL frame with a temporal op", "frame numbers", which);
    }
    {  // twice the same frame and one missing: the count fits, the range does not
        std::vector<cp::Entry> t = clip_table(r, 1, 3, false);
        t[2].frame = t[1].frame;
        refused(cp::make(VSZIP_U8, 8, &cm, 1, t.data(), 3, true), "a frame twice", "a second time", 0);
        t[2].frame = t[1].frame + 2;
        refused(cp::make(VSZIP_U8, 8, &cm, 1, t.data(), 3, true), "a frame missing", "gap", 0);
        const cp::Op pair[2] = {blur, still};  // CombMask with mthresh == 0 is not temporal: the same tables are fine
        CHECK(cp::make(VSZIP_U8, 8, pair, 2, t.data(), 3, true).ok && cp::make(VSZIP_U8, 8, pair, 2, t.data(), 3, false).ok, "a chain without a temporal op needs no clip");
        t[0].frame = INT32_MAX, t[1].frame = INT32_MIN, t[2].frame = 0;  // (no overflow on the way to the refusal)
        refused(cp::make(VSZIP_U8, 8, &cm, 1, t.data(), 3, true), "frames at the ends of int", "gap", 0);
        t[0].frame = INT32_MAX, t[1].frame = INT32_MAX - 1, t[2].frame = INT32_MAX - 2;
        const cp::Plan p = cp::make(VSZIP_U8, 8, &cm, 1, t.data(), 3, true);
        CHECK(p.ok && p.ops[0][0].n2 == 0 && p.ops[0][0].p2 == 2 && p.ops[0][2].p1 == 2 && p.ops[0][2].n2 == 0, "a clip that ends at INT32_MAX");
    }
    // the sample type of every kind, the kind number, params, bits
    for (int kind = -2; kind <= cp::kKinds + 1; ++kind)
        for (int dtype = -1; dtype <= 5; ++dtype)
            for (int at = 0; at < 3; ++at) {
                cp::Op three[3] = {op_of(VSZIP_STAGE_LIMITER), op_of(VSZIP_STAGE_LIMITER), op_of(VSZIP_STAGE_LIMITER)};
                three[at] = op_of(kind, kind == VSZIP_STAGE_CHECKMATE);
                const cp::Plan p = cp::make(dtype, dtype == VSZIP_U8 ? 8 : 16, three, 3, clip.data(), n, true);
                char what[64], need[16];
                snprintf(what, sizeof what, "kind %d on sample type %d as op %d", kind, dtype, at);
                snprintf(need, sizeof need, "op %d", at);
                if (dtype < 0 || dtype > 4) refused(p, what, "sample type", -1);
                else if (kind < 0 || kind >= cp::kKinds) refused(p, what, need, at);
                else if (!takes(kind, dtype)) {
                    refused(p, what, need, at);
                    refused(p, what, "does not take sample type", at);
                } else CHECK(p.ok, "%s is refused: %s", what, p.why.c_str());
            }
    for (int at = 0; at < 3; ++at) {
        cp::Op three[3] = {blur, blur, blur};
        three[at].has_params = false;
        char need[16];
        snprintf(need, sizeof need, "op %d", at);
        refused(cp::make(VSZIP_U16, 16, three, 3, clip.data(), n, false), "NULL params", need, at);
        refused(cp::make(VSZIP_U16, 16, three, 3, clip.data(), n, false), "NULL params", "params is NULL", at);
    }
    for (int kind : {VSZIP_STAGE_MOSQUITO_NR, VSZIP_STAGE_BILATERAL_DITHER}) {
        const cp::Op two[2] = {blur, op_of(kind)};
        for (int bits = 0; bits <= 33; ++bits) {
            const cp::Plan p8 = cp::make(VSZIP_U8, bits, two, 2, clip.data(), n, false), p16 = cp::make(VSZIP_U16, bits, two, 2, clip.data(), n, false);
            if (bits == 8) CHECK(p8.ok, "8 bits on U8");
            else refused(p8, "bits on U8", "bits_per_sample", 1);
            if (bits >= 9 && bits <= 16) CHECK(p16.ok, "%d bits on U16", bits);
            else refused(p16, "bits on U16", "bits_per_sample", 1);
            CHECK(cp::make(VSZIP_F32, bits, two, 2, clip.data(), n, false).ok, "bits are ignored on F32");
            CHECK(cp::make(VSZIP_U16, bits, &blur, 1, clip.data(), n, false).ok, "bits are not looked at without MosquitoNR / BilateralDither");
        }
    }
    // the planes
    for (int i = 0; i < n; ++i) {
        char need[24];
        snprintf(need, sizeof need, "bad plane %d", i);
        for (int how = 0; how < 5; ++how) {
            std::vector<cp::Entry> t = clip;
            if (how == 0) t[i].slot = -1;
            if (how == 1) t[i].slot = 3;
            if (how == 2) t[i].w = 0;
            if (how == 3) t[i].h = -4;
            if (how == 4) t[i].has_planes = false;
            const cp::Plan p = cp::make(VSZIP_U8, 8, ops, 3, t.data(), n, true);
            refused(p, "a bad plane", need, -1);
            CHECK(p.bad_entry == i, "bad plane %d is reported as %d", i, p.bad_entry);
        }
    }
    refused(cp::make(VSZIP_U8, 8, ops, 0, clip.data(), n, true), "no ops", "no ops", -1);
    refused(cp::make(VSZIP_U8, 8, ops, 3, clip.data(), 0, true), "no planes", "no planes", -1);
}

#define LAYOUT_BEGIN(T) printf("struct %s size %zu", #T, sizeof(T))
#define FIELD(T, f) printf(" %s %zu", #f, offsetof(T, f))
#define LAYOUT_END() printf("\n")

static void layouts() {
    LAYOUT_BEGIN(vszip_chain_op); FIELD(vszip_chain_op, kind); FIELD(vszip_chain_op, process); FIELD(vszip_chain_op, params); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_boxblur); FIELD(vszip_chain_boxblur, hradius); FIELD(vszip_chain_boxblur, hpasses); FIELD(vszip_chain_boxblur, vradius); FIELD(vszip_chain_boxblur, vpasses); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_bilateral); FIELD(vszip_chain_bilateral, cfg); FIELD(vszip_chain_bilateral, peak); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_limiter); FIELD(vszip_chain_limiter, lo); FIELD(vszip_chain_limiter, hi); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_clahe); FIELD(vszip_chain_clahe, limit); FIELD(vszip_chain_clahe, tiles_x); FIELD(vszip_chain_clahe, tiles_y); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_comb_mask); FIELD(vszip_chain_comb_mask, cthresh); FIELD(vszip_chain_comb_mask, mthresh); FIELD(vszip_chain_comb_mask, expand); FIELD(vszip_chain_comb_mask, metric); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_comb_mask_mt); FIELD(vszip_chain_comb_mask_mt, thy1); FIELD(vszip_chain_comb_mask_mt, thy2); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_checkmate); FIELD(vszip_chain_checkmate, thr); FIELD(vszip_chain_checkmate, tmax); FIELD(vszip_chain_checkmate, tthr2); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_mosquito_nr); FIELD(vszip_chain_mosquito_nr, strength); FIELD(vszip_chain_mosquito_nr, restore); FIELD(vszip_chain_mosquito_nr, radius); FIELD(vszip_chain_mosquito_nr, chroma); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_deband); FIELD(vszip_chain_deband, per); FIELD(vszip_chain_deband, sample_mode); FIELD(vszip_chain_deband, blur_first); FIELD(vszip_chain_deband, angle_boost); FIELD(vszip_chain_deband, max_angle); FIELD(vszip_chain_deband, max_offset); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_bilateral_dither); FIELD(vszip_chain_bilateral_dither, per); LAYOUT_END();
    LAYOUT_BEGIN(vszip_chain_compress); FIELD(vszip_chain_compress, tables); FIELD(vszip_chain_compress, chroma); LAYOUT_END();
}

int main() {
    static_assert(cp::kKinds == VSZIP_STAGE_COMPRESS + 1 && (int)cp::kCheckmate == VSZIP_STAGE_CHECKMATE && (int)cp::kU32 == VSZIP_U32, "chain_plan.hpp restates the header's numbers");
    sweep();
    refusals();
    layouts();
    printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
