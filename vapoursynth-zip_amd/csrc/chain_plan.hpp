// The plan of a resident chain (vszip_chain_ops, chain.hip): which op filters which table entry, where every entry is read and written, what the
// context's chain buffer holds, and which entries a temporal op takes as the neighbouring frames. Plain C++ (no HIP, no vszip_ctx, no pointers into
// device memory): the input is the ops' kind / process mask / temporal flag and the table's slots, frames and sizes; chain.hip turns the result into
// calls and nothing else, and tests/chain_plan_check.cpp sweeps it on the host.
//
// The scheme. Entry i has writers[i] ops that filter it (those whose process mask names its slot; so every entry of a slot has the same count). Its
// c-th writer (c = 0 ...) reads what writer c - 1 wrote, or the caller's src for c = 0, and writes half c & 1 of the entry's own region of the chain
// buffer, or the caller's dst when it is the last. Writer c - 1 wrote half (c - 1) & 1, the other one, so no op reads memory it writes. A temporal op
// reads neighbouring frames of the same slot: they have been written equally often, so they are read from THEIR half (c - 1) & 1 (or their src) while
// the op writes halves c & 1 (or the callers' dsts): what a temporal op reads, no entry of it writes. Regions of different entries do not overlap, and
// an entry with fewer than two writers has none (src -> dst directly).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace chain_plan {

// the numbers of include/vszip_hip.h (VSZIP_STAGE_*, vszip_dtype), restated so that this header needs nothing else; chain.hip static_asserts them
enum Kind { kBoxBlur = 0, kBilateral, kLimiter, kClahe, kCombMask, kCombMaskMT, kCheckmate, kMosquitoNR, kDeband, kBilateralDither, kCompress, kKinds };
enum DType { kU8 = 0, kU16 = 1, kF16 = 2, kF32 = 3, kU32 = 4 };

inline int sample_bytes(int dtype) {
    switch (dtype) {
        case kU8: return 1;
        case kU16: case kF16: return 2;
        case kF32: case kU32: return 4;
    }
    return 0;
}
inline const char *kind_name(int kind) {
    static const char *const names[kKinds] = {"BoxBlur", "Bilateral", "Limiter", "CLAHE", "CombMask", "CombMaskMT", "Checkmate", "MosquitoNR", "Deband", "BilateralDither", "Compress"};
    return kind >= 0 && kind < kKinds ? names[kind] : "?";
}
// the sample types a kind's entry point serves, as a mask of 1 << dtype. CombMask, CombMaskMT, Checkmate and Compress take no dtype argument
// (8-bit only): the chain is the one place that can refuse them on wider planes, which they would read as bytes.
inline unsigned dtype_mask(int kind) {
    const unsigned u8 = 1u << kU8, u16 = 1u << kU16, f16 = 1u << kF16, f32 = 1u << kF32, u32 = 1u << kU32;
    switch (kind) {
        case kBoxBlur: case kBilateral: return u8 | u16 | f16 | f32;
        case kLimiter: return u8 | u16 | f16 | f32 | u32;
        case kClahe: return u8 | u16;
        case kCombMask: case kCombMaskMT: case kCheckmate: case kCompress: return u8;
        case kDeband: return u16 | f32;
        case kMosquitoNR: case kBilateralDither: return u8 | u16 | f32;
    }
    return 0;
}
inline bool uses_bits(int kind) { return kind == kMosquitoNR || kind == kBilateralDither; }
// bits_per_sample as those two entry points want it: 8 for U8, 9 .. 16 for U16, ignored for F32
inline bool bits_fit(int dtype, int bits) { return dtype == kU8 ? bits == 8 : dtype == kU16 ? (bits >= 9 && bits <= 16) : true; }

struct Op {
    int kind = 0;
    bool process[3] = {false, false, false};
    bool temporal = false;    // Checkmate; CombMask with mthresh > 0
    bool has_params = true;   // the op's params pointer is not NULL
};
struct Entry {
    int slot = 0, frame = 0, w = 0, h = 0;  // frame: ignored when the table has no frame numbers
    bool has_planes = true;                 // src and dst are not NULL
};

enum Where { kSrc = 0, kHalf0 = 1, kHalf1 = 2, kDst = 3 };  // the caller's src, a half of the entry's region of the chain buffer, the caller's dst

struct Step {            // one entry of one op
    int entry = 0;       // index into the table; steps of an op are in table order, which is the order of the compacted per-entry arrays
    int reads = kSrc;    // kSrc | kHalf0 | kHalf1; a temporal op reads its neighbour entries in the same place (their own src / region)
    int writes = kDst;   // kHalf0 | kHalf1 | kDst
    int p2 = -1, p1 = -1, n1 = -1, n2 = -1;  // temporal ops: the entries holding frames n - 2 .. n + 2 of the slot, clamped to fmin .. fmax (p1 is CombMask's previous frame)
};

struct Plan {
    bool ok = false;
    int bad_op = -1, bad_entry = -1;  // what the refusal is about (-1: not about one)
    std::string why;                  // the refusal's text
    std::vector<int> writers;         // per entry
    std::vector<size_t> offset, pitch;  // per entry: its region's start in the chain buffer and the row pitch of its halves, in bytes (256-byte multiples)
    size_t bytes = 0;                 // what the chain buffer must hold
    std::vector<std::vector<Step>> ops;  // per op: its steps (none: the op filters nothing of this table)
    std::vector<int> copies;          // entries no op writes: dst = src when the two differ

    size_t half_bytes(int i, const Entry *e) const { return pitch[i] * (size_t)e[i].h; }
    size_t region_bytes(int i, const Entry *e) const { return writers[i] > 1 ? 2 * half_bytes(i, e) : 0; }
    // where half `where` (kHalf0 | kHalf1) of entry i starts
    size_t half_offset(int i, int where, const Entry *e) const { return offset[i] + (size_t)(where - kHalf0) * half_bytes(i, e); }
};

namespace detail {
inline Plan refuse(Plan &&p, int op, int entry, const std::string &why) {
    p.ok = false;
    p.bad_op = op;
    p.bad_entry = entry;
    p.why = why;
    return std::move(p);
}
inline std::string op_name(int s, int kind) { return "chain: op " + std::to_string(s) + " (" + kind_name(kind) + ")"; }
}  // namespace detail

// have_frames == false: the table has no frame numbers (refused when an op is temporal)
inline Plan make(int dtype, int bits, const Op *ops, int nops, const Entry *e, int n, bool have_frames) {
    using detail::op_name;
    using detail::refuse;
    auto N = [](long v) { return std::to_string(v); };
    Plan p;
    const int bps = sample_bytes(dtype);
    if (bps <= 0) return refuse(std::move(p), -1, -1, "chain: sample type " + N(dtype));
    if (nops <= 0 || n <= 0 || !ops || !e) return refuse(std::move(p), -1, -1, "chain: no ops or no planes");
    for (int i = 0; i < n; ++i)
        if (!e[i].has_planes || e[i].w <= 0 || e[i].h <= 0 || e[i].slot < 0 || e[i].slot > 2) return refuse(std::move(p), -1, i, "chain: bad plane " + N(i));
    bool temporal = false;
    for (int s = 0; s < nops; ++s) {
        const Op &o = ops[s];
        if (o.kind < 0 || o.kind >= kKinds) return refuse(std::move(p), s, -1, "chain: op " + N(s) + ": kind " + N(o.kind));
        if (!o.has_params) return refuse(std::move(p), s, -1, op_name(s, o.kind) + ": params is NULL");
        if (!(dtype_mask(o.kind) >> dtype & 1u)) return refuse(std::move(p), s, -1, op_name(s, o.kind) + " does not take sample type " + N(dtype));
        if (uses_bits(o.kind) && !bits_fit(dtype, bits))
            return refuse(std::move(p), s, -1, op_name(s, o.kind) + ": bits_per_sample " + N(bits) + " does not fit sample type " + N(dtype));
        temporal = temporal || o.temporal;
    }
    // the table as a clip: per slot one contiguous range of frames, each once, one size
    int fmin[3] = {0, 0, 0}, fmax[3] = {0, 0, 0}, count[3] = {0, 0, 0}, first[3] = {-1, -1, -1};
    std::vector<int> at[3];  // per slot: frame - fmin -> entry
    if (temporal) {
        int first_temporal = 0;
        while (!ops[first_temporal].temporal) ++first_temporal;
        if (!have_frames) return refuse(std::move(p), first_temporal, -1, op_name(first_temporal, ops[first_temporal].kind) + " reads neighbouring frames: the table needs frame numbers");
        for (int i = 0; i < n; ++i) {
            const int k = e[i].slot;
            if (first[k] < 0) {
                first[k] = i;
                fmin[k] = fmax[k] = e[i].frame;
            } else {
                if (e[i].w != e[first[k]].w || e[i].h != e[first[k]].h)
                    return refuse(std::move(p), first_temporal, i, op_name(first_temporal, ops[first_temporal].kind) + " reads neighbouring frames: plane " + N(i) + " differs in size from the other planes of slot " + N(k));
                fmin[k] = e[i].frame < fmin[k] ? e[i].frame : fmin[k];
                fmax[k] = e[i].frame > fmax[k] ? e[i].frame : fmax[k];
            }
            ++count[k];
        }
        for (int k = 0; k < 3; ++k) {
            if (!count[k]) continue;
            const long span = (long)fmax[k] - (long)fmin[k] + 1;
            if (span > count[k]) return refuse(std::move(p), first_temporal, -1, op_name(first_temporal, ops[first_temporal].kind) + " reads neighbouring frames: the frame numbers " + N(fmin[k]) + " .. " + N(fmax[k]) + " of slot " + N(k) + " have a gap");
            at[k].assign((size_t)span, -1);  // (span <= count: bounded by the table)
        }
        for (int i = 0; i < n; ++i) {
            int &cell = at[e[i].slot][(size_t)((long)e[i].frame - fmin[e[i].slot])];
            if (cell >= 0) return refuse(std::move(p), first_temporal, i, op_name(first_temporal, ops[first_temporal].kind) + " reads neighbouring frames: plane " + N(i) + " is frame " + N(e[i].frame) + " of slot " + N(e[i].slot) + " a second time");
            cell = i;
        }
        // span <= count and no frame twice: every cell is filled
    }
    // writers and the buffer layout: two dense planes per entry that more than one op writes
    p.writers.assign(n, 0);
    p.offset.assign(n, 0);
    p.pitch.assign(n, 0);
    size_t end = 0;
    for (int i = 0; i < n; ++i) {
        for (int s = 0; s < nops; ++s) p.writers[i] += ops[s].process[e[i].slot] ? 1 : 0;
        p.pitch[i] = ((size_t)e[i].w * bps + 255) & ~(size_t)255;
        p.offset[i] = end;
        end += p.region_bytes(i, e);
    }
    p.bytes = end;
    std::vector<int> written(n, 0);
    p.ops.resize(nops);
    for (int s = 0; s < nops; ++s) {
        const Op &o = ops[s];
        for (int i = 0; i < n; ++i) {
            const int k = e[i].slot;
            if (!o.process[k]) continue;
            Step st;
            st.entry = i;
            const int c = written[i];
            st.reads = c == 0 ? kSrc : kHalf0 + ((c - 1) & 1);
            st.writes = c + 1 == p.writers[i] ? kDst : kHalf0 + (c & 1);
            if (o.temporal) {
                auto nb = [&](long d) {
                    long f = (long)e[i].frame + d;
                    f = f < fmin[k] ? fmin[k] : f > fmax[k] ? fmax[k] : f;
                    return at[k][(size_t)(f - fmin[k])];
                };
                st.p2 = nb(-2), st.p1 = nb(-1), st.n1 = nb(1), st.n2 = nb(2);
            }
            p.ops[s].push_back(st);
        }
        for (const Step &st : p.ops[s]) ++written[st.entry];
    }
    for (int i = 0; i < n; ++i)
        if (p.writers[i] == 0) p.copies.push_back(i);
    p.ok = true;
    return p;
}

}  // namespace chain_plan
