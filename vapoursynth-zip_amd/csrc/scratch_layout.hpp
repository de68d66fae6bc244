// How a filter lays its intermediates out in the context's scratch buffer: a bump layout in bytes. A filter declares its regions once, in order;
// the total (what it reserves) and every pointer (where a region lies) come from the same declaration. Plain C++ (no HIP, no vszip_ctx): the layouts
// of PlaneStats, EEDI3 and SSIMULACRA2 are functions of plain integers below, and tests/scratch_layout_check.cpp sweeps them on the host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace scratch {

// `count` elements of T, `offset` bytes behind the base of the buffer
template <typename T>
struct Region {
    size_t offset = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    size_t end() const { return offset + bytes(); }
    T *in(void *base) const { return reinterpret_cast<T *>(static_cast<char *>(base) + offset); }
};

class Layout {
    size_t end_ = 0;

public:
    // the next region, its start rounded up to `align` bytes; one of no elements takes no space, not even the rounding
    template <typename T>
    Region<T> take(size_t count, size_t align = alignof(T)) {
        if (count == 0) return {end_, 0};
        align_to(align);
        const Region<T> r{end_, count};
        end_ = r.end();
        return r;
    }
    // `times` copies of a layout as one region: copy k of an inner region r lies at r.in(outer.in(base) + k * inner.bytes())
    Region<char> take(const Layout &inner, size_t times, size_t align) { return take<char>(times * inner.bytes(), align); }
    void pad(size_t bytes) { end_ += bytes; }  // space nothing points to
    void align_to(size_t a) { end_ = (end_ + a - 1) / a * a; }
    size_t bytes() const { return end_; }
};

// ---- PlaneStats (planestats.hip: prepare) ---------------------------------------------------------------------------------------------------
struct PlaneStatsScratch {
    Layout all;
    Region<double> partial;               // [block][4]
    Region<uint32_t> hist, bucket, shist;  // per plane; contiguous, cleared with one memset of clear_bytes() from hist
    size_t clear_bytes() const { return shist.end() - hist.offset; }
};
inline PlaneStatsScratch planestats_scratch(size_t blocks, size_t nplanes, size_t hist_words, size_t bucket_words) {
    PlaneStatsScratch s;
    s.partial = s.all.take<double>(blocks * 4);
    s.all.pad(nplanes * 4 * sizeof(double));  // dead: the per-plane results lay here before they moved to pinned host memory
    s.hist = s.all.take<uint32_t>(nplanes * hist_words);
    s.bucket = s.all.take<uint32_t>(nplanes * bucket_words);
    s.shist = s.all.take<uint32_t>(nplanes * 256);
    s.all.pad(256);  // dead tail
    return s;
}

// ---- EEDI3 (eedi3.hip: eedi3_batch) ---------------------------------------------------------------------------------------------------------
struct Eedi3Plane {
    int L, n_src, n_dst, n_interp;  // line length; source, destination and interpolated lines
    bool sclip, mclip;              // the plane has an sclip that vcheck reads / a mask
};
struct Eedi3PlaneScratch {
    Region<float> srcT, dstT, scT;  // horizontal only: the transposed source, destination and sclip
    Region<int> dmap;
    Region<int8_t> pback;
    Region<uint8_t> maskT;  // horizontal only: the transposed mask
};
struct Eedi3Scratch {
    Layout all;
    std::vector<Eedi3PlaneScratch> p;  // by plane index
    Region<float> gline;               // vcheck on lines wider than 8192: two lines per plane
};
// order: the planes' slots (tall planes first); dmap and pback follow it, the transposed planes the plane index. xb: columns per block of the line kernel.
inline Eedi3Scratch eedi3_scratch(const Eedi3Plane *pl, const int *order, int nplanes, bool horizontal, bool vcheck, int tpitch, int xb) {
    Eedi3Scratch s;
    s.p.resize(nplanes);
    int maxL = 0;
    for (int i = 0; i < nplanes; ++i) {
        const Eedi3Plane &g = pl[i];
        maxL = g.L > maxL ? g.L : maxL;
        const size_t on = horizontal ? 1 : 0;
        s.p[i].srcT = s.all.take<float>(on * g.n_src * g.L);
        s.p[i].dstT = s.all.take<float>(on * g.n_dst * g.L);
        s.p[i].scT = s.all.take<float>(vcheck && g.sclip ? on * g.n_dst * g.L : 0);
    }
    for (int k = 0; k < nplanes; ++k) s.p[order[k]].dmap = s.all.take<int>((size_t)pl[order[k]].n_interp * pl[order[k]].L);
    // the back-pointer area is written with 16-byte stores: keep it 256-byte aligned
    const size_t unaligned = s.all.bytes();
    s.all.align_to(256);
    const size_t realign = s.all.bytes() - unaligned;
    for (int k = 0; k < nplanes; ++k) {
        const Eedi3Plane &g = pl[order[k]];
        s.p[order[k]].pback = s.all.take<int8_t>((size_t)g.n_interp * ((g.L + xb - 1) / xb * xb) * tpitch);  // the line kernel stores whole blocks of xb columns
    }
    for (int i = 0; i < nplanes; ++i) {
        s.p[i].maskT = s.all.take<uint8_t>(horizontal && pl[i].mclip ? (size_t)pl[i].n_src * pl[i].L : 0);
        s.all.pad((256 - s.p[i].maskT.count % 256) % 256);  // a multiple of 256 bytes each (behind the back-pointers: not 256-byte aligned itself)
    }
    s.all.pad(4096 - realign);  // dead tail: 4096 bytes, of which the realignment above took its share
    s.all.align_to(256);
    s.gline = s.all.take<float>(vcheck && maxL > 8192 ? (size_t)nplanes * 2 * ((maxL + 63) & ~63) : 0);
    return s;
}

// ---- SSIMULACRA2 (ssimulacra2.hip: vszip_ssimulacra2_src) -----------------------------------------------------------------------------------
struct SsimTables {  // the pointer tables: staged in the pinned scalars buffer in this layout, copied to the scratch buffer in one piece
    Layout all;
    Region<char> tab, pyr;  // [scale][pair] PairPtrs, [pair] PyrPair
};
struct SsimPair {  // one pair's float planes
    Layout all;
    // XYB of scales 0 and 1, linear RGB of scale 2, XYB of one later scale at a time, RGB of scales 3 and 4, and the two frames' full-size linear RGB
    // between the colour pre-stage and the pyramid pass (rgb_stage only)
    Region<float> x0, x1, r2, xs, r3, r4, rgb;
};
struct SsimScratch {
    Layout all;
    Region<double> partial;  // [pair][18][tile][6]
    size_t avg_bytes;        // [pair][18][6] doubles, rounded: what the final kernel writes to the scalars buffer (and dead space of that size here)
    SsimTables tables;
    Region<char> tables_at;  // `tables`, once
    SsimPair pair;
    Region<char> pairs;      // `pair`, npairs times
};
// npx: samples of a plane at scales 0 ... 4; nneed0 / nneed1: XYB planes scales 0 / 1 keep
inline SsimScratch ssim_scratch(const size_t *npx, int nneed0, int nneed1, size_t npairs, size_t tiles0, bool rgb_stage, size_t scales, size_t pairptrs_bytes,
                                size_t pyrpair_bytes) {
    SsimScratch s;
    s.tables.tab = s.tables.all.take<char>(scales * npairs * pairptrs_bytes, 256);
    s.tables.pyr = s.tables.all.take<char>(npairs * pyrpair_bytes, 256);
    s.tables.all.align_to(256);
    // every region starts on a multiple of 4 floats: the linear-RGB planes are written and read with 16-byte accesses (6 npx[3] + 6 npx[4] is 2 mod 4
    // for e.g. 1924 x 1080)
    SsimPair &f = s.pair;
    f.x0 = f.all.take<float>(2 * (size_t)nneed0 * npx[0], 16);
    f.x1 = f.all.take<float>(2 * (size_t)nneed1 * npx[1], 16);
    f.r2 = f.all.take<float>(6 * npx[2], 16);
    f.xs = f.all.take<float>(6 * npx[2], 16);
    f.r3 = f.all.take<float>(6 * npx[3], 16);
    f.r4 = f.all.take<float>(6 * npx[4], 16);
    f.rgb = f.all.take<float>(rgb_stage ? 6 * npx[0] : 0, 16);
    f.all.align_to(256);

    s.partial = s.all.take<double>(npairs * 18 * tiles0 * 6, 256);
    s.all.align_to(256);
    s.avg_bytes = (npairs * 18 * 6 * sizeof(double) + 255) & ~(size_t)255;
    s.all.pad(s.avg_bytes);  // dead: the averages go to the scalars buffer
    s.tables_at = s.all.take(s.tables.all, 1, 256);
    s.pairs = s.all.take(s.pair.all, npairs, 256);
    s.all.pad(1024);  // dead tail
    return s;
}

}  // namespace scratch
