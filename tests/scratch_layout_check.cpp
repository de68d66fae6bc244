// Host check of the scratch layouts (vapoursynth-zip_amd/csrc/scratch_layout.hpp), run by tests/test_scratch_layout_host.py under
// AddressSanitizer + UndefinedBehaviorSanitizer. (1) The layout type: regions are sequential and never overlap, every offset is a multiple of its
// alignment, bytes() is the end of the last region or pad, regions of no elements take no space, a nested layout's regions lie at
// base + outer offset + inner offset. (2) The layouts of PlaneStats, EEDI3 and SSIMULACRA2 against the formulas these filters computed by hand
// before the layouts existed - one expression for the size, another for the pointers - spelled out here as they stood: every region offset and the
// total, over a sweep of shapes. (A region of no elements has no bytes whose place could matter: its offset is not compared.)
#include <algorithm>
#include <cstdio>
#include <vector>

#include "scratch_layout.hpp"

using scratch::Layout;
using scratch::Region;

static int failures = 0;
static long checked = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        ++checked;                                \
        if (!(cond)) {                            \
            if (++failures <= 20) {               \
                std::printf("FAIL %s: ", #cond);  \
                std::printf(__VA_ARGS__);         \
                std::printf("\n");                \
            }                                     \
        }                                         \
    } while (0)

// ---- the layout type ------------------------------------------------------------------------------------------------------------------------
struct Seen {
    size_t offset, bytes, align;
};
template <typename T>
static Region<T> take_checked(Layout &l, std::vector<Seen> &seen, size_t count, size_t align) {
    const size_t before = l.bytes();
    const Region<T> r = l.take<T>(count, align);
    if (count == 0) {
        CHECK(l.bytes() == before && r.offset == before && r.bytes() == 0, "an empty region moved the end from %zu to %zu", before, l.bytes());
        return r;
    }
    CHECK(r.offset % align == 0, "offset %zu is not a multiple of %zu", r.offset, align);
    CHECK(r.offset >= before && r.offset - before < align, "offset %zu behind an end of %zu, alignment %zu", r.offset, before, align);
    CHECK(r.count == count && r.bytes() == count * sizeof(T) && r.end() == r.offset + count * sizeof(T), "region of %zu elements: %zu bytes", count, r.bytes());
    CHECK(l.bytes() == r.end(), "bytes() %zu is not the end of the last region %zu", l.bytes(), r.end());
    for (const Seen &s : seen) CHECK(s.offset + s.bytes <= r.offset, "region at %zu overlaps the one at %zu + %zu", r.offset, s.offset, s.bytes);
    seen.push_back({r.offset, r.bytes(), align});
    return r;
}

static void check_type() {
    const size_t counts[] = {0, 1, 3, 64, 257, 100000};
    const size_t aligns[] = {1, 4, 16, 256, 4096};
    for (size_t c0 : counts)
        for (size_t c1 : counts)
            for (size_t c2 : counts)
                for (size_t a1 : aligns)
                    for (size_t a2 : aligns) {
                        Layout l;
                        std::vector<Seen> seen;
                        CHECK(l.bytes() == 0, "an empty layout of %zu bytes", l.bytes());
                        take_checked<char>(l, seen, c0, 1);
                        take_checked<double>(l, seen, c1, std::max(a1, alignof(double)));
                        const size_t e = l.bytes();
                        l.pad(c2 % 300);
                        CHECK(l.bytes() == e + c2 % 300, "pad(%zu) moved the end from %zu to %zu", c2 % 300, e, l.bytes());
                        take_checked<float>(l, seen, c2, std::max(a2, alignof(float)));
                        const size_t e2 = l.bytes();
                        l.align_to(a1);
                        CHECK(l.bytes() % a1 == 0 && l.bytes() >= e2 && l.bytes() - e2 < a1, "align_to(%zu) moved the end from %zu to %zu", a1, e2, l.bytes());
                        take_checked<uint32_t>(l, seen, c1, 4);
                    }
    // pointers: a region's, and a nested layout's taken several times
    alignas(256) static char buffer[1 << 16];
    Layout inner;
    std::vector<Seen> seen_in, seen_out;
    const Region<float> ia = take_checked<float>(inner, seen_in, 5, 16);
    const Region<uint8_t> ib = take_checked<uint8_t>(inner, seen_in, 7, 1);
    const Region<double> ic = take_checked<double>(inner, seen_in, 3, 64);
    inner.align_to(256);
    Layout outer;
    take_checked<int>(outer, seen_out, 9, 4);
    const size_t before = outer.bytes();
    const Region<char> nest = outer.take(inner, 3, 256);
    CHECK(nest.offset == (before + 255) / 256 * 256 && nest.count == 3 * inner.bytes() && outer.bytes() == nest.end(), "nested region at %zu, %zu bytes", nest.offset, nest.count);
    const Region<int> tail = take_checked<int>(outer, seen_out, 2, 4);
    CHECK(tail.offset == nest.end(), "the region behind the nested one at %zu, not %zu", tail.offset, nest.end());
    CHECK(outer.bytes() <= sizeof buffer, "test buffer too small");
    for (size_t k = 0; k < 3; ++k) {
        char *copy = nest.in(buffer) + k * inner.bytes();
        CHECK(reinterpret_cast<char *>(ia.in(copy)) == buffer + nest.offset + k * inner.bytes() + ia.offset, "nested float region, copy %zu", k);
        CHECK(reinterpret_cast<char *>(ib.in(copy)) == buffer + nest.offset + k * inner.bytes() + ib.offset, "nested byte region, copy %zu", k);
        CHECK(reinterpret_cast<char *>(ic.in(copy)) == buffer + nest.offset + k * inner.bytes() + ic.offset, "nested double region, copy %zu", k);
        ic.in(copy)[2] = 1.0;  // (the sanitizers watch these: inside the buffer, aligned for the type)
        ia.in(copy)[4] = 1.0f;
    }
    tail.in(buffer)[1] = 1;
    const Region<int> none = outer.take<int>(0, 4096);
    CHECK(none.in(buffer) == reinterpret_cast<int *>(buffer + outer.bytes()), "an empty region points at the end");
}

// a region of at least one element lies where the hand-written carve put it
#define SAME(region, want, ...) CHECK((region).count == 0 || (region).offset == (want), __VA_ARGS__)

// ---- PlaneStats: planestats.hip, prepare() ---------------------------------------------------------------------------------------------------
static void check_planestats() {
    constexpr int kHistWords = 4096, kBucketWords = 16;
    for (int nplanes = 1; nplanes <= 192; ++nplanes)
        for (int h = 1; h <= 2160; ++h) {
            // every plane h rows, except that every third one has half of them (a subsampled clip)
            int blocks = 0;
            for (int i = 0; i < nplanes; ++i) blocks += ((i % 3 ? (h + 1) / 2 : h) + 8 - 1) / 8;
            // as it stood:
            const size_t need = (size_t)blocks * 4 * sizeof(double) + (size_t)nplanes * (kHistWords + kBucketWords + 256) * sizeof(uint32_t) + (size_t)nplanes * 4 * sizeof(double) + 256;
            size_t p = 0;
            const size_t partial = p;
            p += (size_t)blocks * 4 * sizeof(double);
            p += (size_t)nplanes * 4 * sizeof(double);
            const size_t hist = p;
            p += (size_t)nplanes * kHistWords * sizeof(uint32_t);
            const size_t bucket = p;
            p += (size_t)nplanes * kBucketWords * sizeof(uint32_t);
            const size_t shist = p;
            const size_t cleared = (size_t)nplanes * (kHistWords + kBucketWords + 256) * sizeof(uint32_t);

            const scratch::PlaneStatsScratch s = scratch::planestats_scratch((size_t)blocks, (size_t)nplanes, kHistWords, kBucketWords);
            CHECK(s.all.bytes() == need, "planestats %d planes, %d blocks: %zu bytes, not %zu", nplanes, blocks, s.all.bytes(), need);
            SAME(s.partial, partial, "planestats %d planes, %d blocks: partial at %zu", nplanes, blocks, s.partial.offset);
            SAME(s.hist, hist, "planestats %d planes, %d blocks: hist at %zu, not %zu", nplanes, blocks, s.hist.offset, hist);
            SAME(s.bucket, bucket, "planestats %d planes, %d blocks: bucket at %zu, not %zu", nplanes, blocks, s.bucket.offset, bucket);
            SAME(s.shist, shist, "planestats %d planes, %d blocks: shist at %zu, not %zu", nplanes, blocks, s.shist.offset, shist);
            CHECK(s.clear_bytes() == cleared && s.shist.end() + 256 == need, "planestats %d planes: clears %zu bytes, not %zu", nplanes, s.clear_bytes(), cleared);
        }
}

// ---- EEDI3: eedi3.hip, eedi3_batch() ---------------------------------------------------------------------------------------------------------
static void check_eedi3_case(const std::vector<scratch::Eedi3Plane> &geo, bool horizontal, int vcheck, int tpitch, const char *what) {
    constexpr int kXB = 64;
    const int nplanes = (int)geo.size();
    // the plane slots, as eedi3_batch orders them: tall planes first
    std::vector<int> order(nplanes);
    {
        int ntall = 0, max_interp = 0;
        for (int i = 0; i < nplanes; ++i) max_interp = std::max(max_interp, geo[i].n_interp);
        for (int i = 0; i < nplanes; ++i)
            if (4 * geo[i].n_interp >= 3 * max_interp) order[ntall++] = i;
        int k = ntall;
        for (int i = 0; i < nplanes; ++i)
            if (4 * geo[i].n_interp < 3 * max_interp) order[k++] = i;
    }
    // as it stood:
    struct Off {
        size_t srcT, dstT, scT, mT, dmap, pback;
    };
    std::vector<Off> off(nplanes);
    size_t fl = 0, pb = 0, dm = 0, mb = 0;
    for (int i = 0; i < nplanes; ++i) {
        const scratch::Eedi3Plane &g = geo[i];
        if (horizontal) {
            off[i].srcT = fl;
            fl += (size_t)g.n_src * g.L;
            off[i].dstT = fl;
            fl += (size_t)g.n_dst * g.L;
            off[i].scT = fl;
            if (vcheck > 0 && g.sclip) fl += (size_t)g.n_dst * g.L;
            off[i].mT = mb;
            if (g.mclip) mb += (((size_t)g.n_src * g.L) + 255) & ~(size_t)255;
        }
        pb += (size_t)g.n_interp * ((g.L + kXB - 1) / kXB * kXB) * tpitch;
        dm += (size_t)g.n_interp * g.L;
    }
    size_t bytes = (fl * sizeof(float) + dm * sizeof(int) + pb + mb + 4096 + 255) & ~(size_t)255;
    const size_t gline_off = bytes;
    int maxL = 0;
    for (int i = 0; i < nplanes; ++i) maxL = std::max(maxL, geo[i].L);
    if (vcheck > 0 && maxL > 8192) bytes += (size_t)nplanes * 2 * ((maxL + 63) & ~63) * sizeof(float);
    const size_t dbase = fl * sizeof(float);
    const size_t pb_off = (fl * sizeof(float) + dm * sizeof(int) + 255) & ~(size_t)255;
    const size_t mbase = pb_off + pb;
    size_t dmo = 0, pbo = 0;
    for (int slot = 0; slot < nplanes; ++slot) {
        const scratch::Eedi3Plane &g = geo[order[slot]];
        off[order[slot]].dmap = dbase + dmo * sizeof(int);
        off[order[slot]].pback = pb_off + pbo;
        dmo += (size_t)g.n_interp * g.L;
        pbo += (size_t)g.n_interp * ((g.L + kXB - 1) / kXB * kXB) * tpitch;
    }

    const scratch::Eedi3Scratch s = scratch::eedi3_scratch(geo.data(), order.data(), nplanes, horizontal, vcheck > 0, tpitch, kXB);
    CHECK(s.all.bytes() == bytes, "%s: %zu bytes, not %zu", what, s.all.bytes(), bytes);
    CHECK((int)s.p.size() == nplanes, "%s: %zu planes", what, s.p.size());
    for (int i = 0; i < nplanes; ++i) {
        const scratch::Eedi3PlaneScratch &q = s.p[i];
        if (horizontal) {
            CHECK(q.srcT.count > 0 && q.dstT.count > 0 && (q.scT.count > 0) == (vcheck > 0 && geo[i].sclip) && (q.maskT.count > 0) == geo[i].mclip, "%s plane %d: a transposed plane is missing", what, i);
            SAME(q.srcT, off[i].srcT * sizeof(float), "%s plane %d: srcT at %zu", what, i, q.srcT.offset);
            SAME(q.dstT, off[i].dstT * sizeof(float), "%s plane %d: dstT at %zu", what, i, q.dstT.offset);
            SAME(q.scT, off[i].scT * sizeof(float), "%s plane %d: scT at %zu", what, i, q.scT.offset);
            SAME(q.maskT, mbase + off[i].mT, "%s plane %d: maskT at %zu, not %zu", what, i, q.maskT.offset, mbase + off[i].mT);
        } else {
            CHECK(q.srcT.count + q.dstT.count + q.scT.count + q.maskT.count == 0, "%s plane %d: transposed planes in a vertical call", what, i);
        }
        CHECK(q.dmap.count > 0 && q.pback.count > 0, "%s plane %d: no dmap or pback", what, i);
        SAME(q.dmap, off[i].dmap, "%s plane %d: dmap at %zu, not %zu", what, i, q.dmap.offset, off[i].dmap);
        SAME(q.pback, off[i].pback, "%s plane %d: pback at %zu, not %zu", what, i, q.pback.offset, off[i].pback);
    }
    CHECK((s.gline.count > 0) == (vcheck > 0 && maxL > 8192), "%s: gline of %zu floats", what, s.gline.count);
    CHECK(s.gline.offset == gline_off && s.gline.end() == bytes, "%s: gline at %zu, not %zu", what, s.gline.offset, gline_off);  // (eedi3_batch takes the pointer whenever maxL > 8192)
}

static void check_eedi3() {
    const int lens[] = {5, 63, 64, 65, 127, 128, 129, 1920, 8191, 8192, 8193};  // around the 64-column blocks of the line kernel, and the gline threshold
    const int srcs[] = {2, 6, 34, 270, 1080};
    const unsigned masks[] = {0u, ~0u, 0x15u, 0x2Au, 0x0Bu, 0x34u};  // which planes have an sclip / a mask
    const int tpitches[] = {2 * 20 + 1, 2 * 31 + 1, 4 * 40 + 1};
    char what[160];
    for (int horizontal = 0; horizontal < 2; ++horizontal)
        for (int dh = 0; dh < 2; ++dh)
            for (int vcheck : {0, 2})
                for (int nplanes = 1; nplanes <= 6; ++nplanes)
                    for (int a = 0; a < (int)(sizeof lens / sizeof *lens); ++a)
                        for (int b = 0; b < (int)(sizeof srcs / sizeof *srcs); ++b)
                            for (unsigned sm : masks)
                                for (unsigned mm : masks)
                                    for (int tpitch : tpitches) {
                                        std::vector<scratch::Eedi3Plane> geo(nplanes);
                                        for (int i = 0; i < nplanes; ++i) {  // mixed sizes: another line length per plane, every other plane half as many lines
                                            scratch::Eedi3Plane &g = geo[i];
                                            g.L = lens[(a + 3 * i) % (int)(sizeof lens / sizeof *lens)];
                                            g.n_src = srcs[(b + i) % (int)(sizeof srcs / sizeof *srcs)];
                                            if (i & 1) g.n_src = std::max(2, (g.n_src / 2) & ~1);
                                            g.n_dst = dh ? 2 * g.n_src : g.n_src;
                                            g.n_interp = dh ? g.n_src : g.n_src / 2;
                                            g.sclip = (sm >> i) & 1;
                                            g.mclip = (mm >> i) & 1;
                                        }
                                        std::snprintf(what, sizeof what, "eedi3 %s dh=%d vcheck=%d planes=%d L0=%d src0=%d sclips=%x masks=%x tpitch=%d", horizontal ? "H" : "V", dh, vcheck,
                                                      nplanes, geo[0].L, geo[0].n_src, sm & 63, mm & 63, tpitch);
                                        check_eedi3_case(geo, horizontal != 0, vcheck, tpitch, what);
                                    }
}

// ---- SSIMULACRA2: ssimulacra2.hip, vszip_ssimulacra2_src() -----------------------------------------------------------------------------------
static void check_ssim_case(int w, int h, int npairs, bool split, bool split_row, int nneed0, int nneed1, size_t sizeof_PairPtrs, size_t sizeof_PyrPair) {
    constexpr int kScales = 5, TW = 56, TH = 32;
    int sw[kScales + 1], sh[kScales + 1];
    sw[0] = w;
    sh[0] = h;
    for (int s = 1; s <= kScales; ++s) {
        sw[s] = (sw[s - 1] + 1) / 2;
        sh[s] = (sh[s - 1] + 1) / 2;
    }
    size_t npx[kScales + 1];
    for (int s = 0; s <= kScales; ++s) npx[s] = (size_t)sw[s] * sh[s];
    const int nneed[2] = {nneed0, nneed1};
    const int tiles0 = ((w + TW - 1) / TW) * ((h + TH - 1) / TH);
    // as it stood:
    auto al4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    const size_t f_x0 = al4(2 * nneed[0] * npx[0]), f_x1 = al4(2 * nneed[1] * npx[1]), f_r2 = al4(6 * npx[2]), f_xs = al4(6 * npx[2]), f_r3 = al4(6 * npx[3]), f_r4 = al4(6 * npx[4]);
    const size_t f_rgb = (split || split_row) ? 6 * npx[0] : 0;
    const size_t f_pair = (f_x0 + f_x1 + f_r2 + f_xs + f_r3 + f_r4 + f_rgb + 63) & ~(size_t)63;
    const size_t bytes_part = ((size_t)npairs * 18 * tiles0 * 6 * sizeof(double) + 255) & ~(size_t)255;
    const size_t bytes_avg = ((size_t)npairs * 18 * 6 * sizeof(double) + 255) & ~(size_t)255;
    const size_t bytes_tab = ((size_t)kScales * npairs * sizeof_PairPtrs + 255) & ~(size_t)255;
    const size_t bytes_pyr = ((size_t)npairs * sizeof_PyrPair + 255) & ~(size_t)255;
    const size_t need = bytes_part + bytes_avg + bytes_tab + bytes_pyr + (size_t)npairs * f_pair * sizeof(float) + 1024;
    const size_t partial = 0, tab_dev = bytes_part + bytes_avg, pyr_dev = bytes_part + bytes_avg + bytes_tab, fbase = bytes_part + bytes_avg + bytes_tab + bytes_pyr;
    const size_t scalars = std::max(bytes_avg, bytes_tab + bytes_pyr);

    const scratch::SsimScratch s = scratch::ssim_scratch(npx, nneed0, nneed1, (size_t)npairs, (size_t)tiles0, split || split_row, kScales, sizeof_PairPtrs, sizeof_PyrPair);
    char what[160];
    std::snprintf(what, sizeof what, "ssim %dx%d pairs=%d split=%d/%d need=%d,%d sizes=%zu,%zu", w, h, npairs, (int)split, (int)split_row, nneed0, nneed1, sizeof_PairPtrs, sizeof_PyrPair);
    CHECK(s.all.bytes() == need, "%s: %zu bytes, not %zu", what, s.all.bytes(), need);
    CHECK(std::max(s.avg_bytes, s.tables.all.bytes()) == scalars && s.tables.all.bytes() == bytes_tab + bytes_pyr, "%s: %zu bytes of scalars, not %zu", what, std::max(s.avg_bytes, s.tables.all.bytes()), scalars);
    SAME(s.partial, partial, "%s: partial at %zu", what, s.partial.offset);
    CHECK(s.tables_at.count == s.tables.all.bytes() && s.pairs.count == (size_t)npairs * s.pair.all.bytes(), "%s: nested regions of %zu and %zu bytes", what, s.tables_at.count, s.pairs.count);
    // in the scratch buffer, and in the pinned buffer the tables are staged in (there from offset 0)
    CHECK(s.tables_at.offset + s.tables.tab.offset == tab_dev && s.tables.tab.offset == 0, "%s: tab at %zu, not %zu", what, s.tables_at.offset + s.tables.tab.offset, tab_dev);
    CHECK(s.tables_at.offset + s.tables.pyr.offset == pyr_dev && s.tables.pyr.offset == bytes_tab, "%s: pyr at %zu, not %zu", what, s.tables_at.offset + s.tables.pyr.offset, pyr_dev);
    CHECK(s.pair.all.bytes() == f_pair * sizeof(float), "%s: %zu bytes a pair, not %zu", what, s.pair.all.bytes(), f_pair * sizeof(float));
    for (int pair = 0; pair < npairs; ++pair) {
        const size_t x0 = fbase / sizeof(float) + (size_t)pair * f_pair, x1 = x0 + f_x0, r2 = x1 + f_x1, xs = r2 + f_r2, r3 = xs + f_xs, r4 = r3 + f_r3, rgb = r4 + f_r4;
        const size_t at = s.pairs.offset + (size_t)pair * s.pair.all.bytes();
        const Region<float> *got[] = {&s.pair.x0, &s.pair.x1, &s.pair.r2, &s.pair.xs, &s.pair.r3, &s.pair.r4, &s.pair.rgb};
        const size_t want[] = {x0, x1, r2, xs, r3, r4, rgb};
        const char *names[] = {"x0", "x1", "r2", "xs", "r3", "r4", "rgb"};
        for (int k = 0; k < 7; ++k) {
            CHECK(got[k]->count == 0 || at + got[k]->offset == want[k] * sizeof(float), "%s pair %d: %s at %zu, not %zu", what, pair, names[k], at + got[k]->offset, want[k] * sizeof(float));
            CHECK(got[k]->count == 0 || (at + got[k]->offset) % 16 == 0, "%s pair %d: %s at %zu is not 16-byte aligned", what, pair, names[k], at + got[k]->offset);
        }
        CHECK((s.pair.rgb.count > 0) == (split || split_row) && s.pair.r2.count == 6 * npx[2] && s.pair.x0.count == 2 * (size_t)nneed0 * npx[0], "%s: region sizes", what);
    }
}

static void check_ssim() {
    std::vector<std::pair<int, int>> sizes = {{1924, 1080}, {1920, 1080}, {3840, 2160}, {1921, 1081}, {1001, 999}, {255, 257}, {720, 481}};
    for (int w = 8; w <= 72; ++w)
        for (int h = 8; h <= 40; h += (w % 3) + 1) sizes.push_back({w, h});
    for (const auto &wh : sizes)
        for (int npairs : {1, 2, 9})
            for (int split = 0; split < 2; ++split)
                for (int split_row = 0; split_row < 2; ++split_row)
                    for (int nneed0 = 0; nneed0 <= 3; ++nneed0)  // skip_of(plane, scale).all() over three planes: a scale keeps 0 ... 3 of them
                        for (int nneed1 = 0; nneed1 <= 3; ++nneed1) {
                            check_ssim_case(wh.first, wh.second, npairs, split != 0, split_row != 0, nneed0, nneed1, 144, 240);  // 18 and 30 pointers: PairPtrs, PyrPair
                            if (nneed0 == 3) check_ssim_case(wh.first, wh.second, npairs, split != 0, split_row != 0, nneed0, nneed1, 104, 8);
                        }
}

int main() {
    check_type();
    check_planestats();
    check_eedi3();
    check_ssim();
    std::printf("%ld checks, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
