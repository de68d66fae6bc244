// vszip_chain_ops / vszip_chain_run: several pixel-filter stages over one table of resident planes in ONE call — what a host
// does for a script that chains vszip filters (clip.vszip.Bilateral().vszip.BoxBlur()...): upload once, run every
// stage on the device, download once. Every entry point of this library already works on device pointers, so
// a chain is a sequence of calls on one context; this one adds the intermediate planes (a grow-only buffer of the
// context, two planes per table entry, ping-pong) and the bookkeeping of which stage wrote which plane, so that
// the host side needs no device allocations of its own. Stages follow the reference's plane semantics: a stage
// filters the planes it is told to and passes the others through (newVideoFrame2's plane copy,
// src/vapoursynth/boxblur.zig:38).
// The bookkeeping is chain_plan.hpp (plain C++: validation, writer counts, buffer layout, who reads and writes where, the temporal ops'
// neighbour entries); this file checks the pointers inside the ops' params, reserves the buffer and turns the plan into calls.
#include <vector>

#include "chain_plan.hpp"
#include "common.hpp"

namespace cp = chain_plan;
static_assert(cp::kBoxBlur == VSZIP_STAGE_BOXBLUR && cp::kBilateral == VSZIP_STAGE_BILATERAL && cp::kLimiter == VSZIP_STAGE_LIMITER && cp::kClahe == VSZIP_STAGE_CLAHE &&
                  cp::kCombMask == VSZIP_STAGE_COMB_MASK && cp::kCombMaskMT == VSZIP_STAGE_COMB_MASK_MT && cp::kCheckmate == VSZIP_STAGE_CHECKMATE &&
                  cp::kMosquitoNR == VSZIP_STAGE_MOSQUITO_NR && cp::kDeband == VSZIP_STAGE_DEBAND && cp::kBilateralDither == VSZIP_STAGE_BILATERAL_DITHER &&
                  cp::kCompress == VSZIP_STAGE_COMPRESS,
              "chain_plan.hpp restates the VSZIP_STAGE_ numbers");
static_assert((int)cp::kU8 == VSZIP_U8 && (int)cp::kU16 == VSZIP_U16 && (int)cp::kF16 == VSZIP_F16 && (int)cp::kF32 == VSZIP_F32 && (int)cp::kU32 == VSZIP_U32, "chain_plan.hpp restates vszip_dtype");

namespace {

template <typename T>
const T &params_of(const vszip_chain_op &op) { return *static_cast<const T *>(op.params); }

// entries idx[] of a per-entry array (NULL stays NULL)
template <typename T>
const T *gather(std::vector<T> &out, const T *all, const std::vector<cp::Step> &steps) {
    if (!all) return nullptr;
    out.resize(steps.size());
    for (size_t k = 0; k < steps.size(); ++k) out[k] = all[steps[k].entry];
    return out.data();
}

// a NULL pointer inside an op's params where its entry point takes none: refused before anything is queued. `used`: slots of which the op processes an entry
const char *missing_pointer(const vszip_chain_op &op, const bool used[3], int *slot) {
    *slot = -1;
    switch (op.kind) {
        case VSZIP_STAGE_BILATERAL:
            for (int k = 0; k < 3; ++k)
                if (used[k] && !params_of<vszip_chain_bilateral>(op).cfg[k]) {
                    *slot = k;
                    return "Bilateral configuration";
                }
            return nullptr;
        case VSZIP_STAGE_MOSQUITO_NR: {
            const auto &m = params_of<vszip_chain_mosquito_nr>(op);
            return !m.strength ? "strength" : !m.restore ? "restore" : !m.radius ? "radius" : nullptr;
        }
        case VSZIP_STAGE_DEBAND: return params_of<vszip_chain_deband>(op).per ? nullptr : "per";
        case VSZIP_STAGE_BILATERAL_DITHER: return params_of<vszip_chain_bilateral_dither>(op).per ? nullptr : "per";
        case VSZIP_STAGE_COMPRESS: return params_of<vszip_chain_compress>(op).tables ? nullptr : "tables";
    }
    return nullptr;
}

}  // namespace

VSZIP_EXPORT int vszip_chain_ops(vszip_ctx *ctx, int dtype, int bits_per_sample, const vszip_chain_op *ops, int nops, const vszip_plane *planes, const int *plane_slot,
                                 const int *frame, int nplanes) {
    if (!ctx || !ops || !planes || !plane_slot || nops <= 0 || nplanes <= 0) return VSZIP_ERR_ARG;
    const int bps = vszip_dtype_size(dtype);
    if (bps <= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "chain: sample type %d", dtype);
    VSZIP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // ---- the plan: everything that can be refused is refused here, before the first launch
    std::vector<cp::Op> pops(nops);
    for (int s = 0; s < nops; ++s) {
        pops[s].kind = ops[s].kind;
        for (int k = 0; k < 3; ++k) pops[s].process[k] = ops[s].process[k] != 0;
        pops[s].has_params = ops[s].params != nullptr;
        pops[s].temporal = pops[s].has_params && (ops[s].kind == VSZIP_STAGE_CHECKMATE || (ops[s].kind == VSZIP_STAGE_COMB_MASK && params_of<vszip_chain_comb_mask>(ops[s]).mthresh > 0));
    }
    std::vector<cp::Entry> ent(nplanes);
    for (int i = 0; i < nplanes; ++i) {
        ent[i].slot = plane_slot[i];
        ent[i].frame = frame ? frame[i] : 0;
        ent[i].w = planes[i].w;
        ent[i].h = planes[i].h;
        ent[i].has_planes = planes[i].src && planes[i].dst;
    }
    const cp::Plan plan = cp::make(dtype, bits_per_sample, pops.data(), nops, ent.data(), nplanes, frame != nullptr);
    if (!plan.ok) return vszip_set_error(ctx, VSZIP_ERR_ARG, "%s", plan.why.c_str());
    for (int s = 0; s < nops; ++s) {
        bool used[3] = {false, false, false};
        for (const cp::Step &st : plan.ops[s]) used[plane_slot[st.entry]] = true;
        int slot;
        if (const char *what = missing_pointer(ops[s], used, &slot)) {
            if (slot >= 0) return vszip_set_error(ctx, VSZIP_ERR_ARG, "chain: op %d has no %s for plane slot %d", s, what, slot);
            return vszip_set_error(ctx, VSZIP_ERR_ARG, "chain: op %d (%s): %s is NULL", s, cp::kind_name(ops[s].kind), what);
        }
    }
    int rc = vszip_reserve(ctx, ctx->chain_buf, plan.bytes, vszip_scratch_want(plan.bytes), "chain buffer");
    if (rc != VSZIP_OK) return rc;
    char *buf = static_cast<char *>(ctx->chain_buf.ptr);
    // where entry i lies for a reader / a writer
    auto place = [&](int i, int where, const void **ptr, ptrdiff_t *stride) {
        if (where == cp::kSrc) {
            *ptr = planes[i].src;
            *stride = planes[i].src_stride;
        } else if (where == cp::kDst) {
            *ptr = planes[i].dst;
            *stride = planes[i].dst_stride;
        } else {
            *ptr = buf + plan.half_offset(i, where, ent.data());
            *stride = (ptrdiff_t)(plan.pitch[i] / bps);
        }
    };
    // ---- the calls
    std::vector<vszip_plane> tab;
    for (int s = 0; s < nops; ++s) {
        const std::vector<cp::Step> &steps = plan.ops[s];
        if (steps.empty()) continue;
        const vszip_chain_op &op = ops[s];
        const int n = (int)steps.size();
        tab.resize(n);
        for (int k = 0; k < n; ++k) {
            const cp::Step &st = steps[k];
            vszip_plane p = planes[st.entry];
            const void *d;
            place(st.entry, st.reads, &p.src, &p.src_stride);
            place(st.entry, st.writes, &d, &p.dst_stride);
            p.dst = const_cast<void *>(d);
            p.ref = nullptr;
            p.ref_stride = 0;
            tab[k] = p;
        }
        switch (op.kind) {
            case VSZIP_STAGE_BOXBLUR: {
                const auto &a = params_of<vszip_chain_boxblur>(op);
                rc = vszip_boxblur(ctx, dtype, tab.data(), n, a.hradius, a.hpasses, a.vradius, a.vpasses);
                break;
            }
            case VSZIP_STAGE_BILATERAL: {
                const auto &a = params_of<vszip_chain_bilateral>(op);
                std::vector<const vszip_bilateral_cfg *> cfgs(n);
                for (int k = 0; k < n; ++k) cfgs[k] = a.cfg[plane_slot[steps[k].entry]];
                rc = vszip_bilateral(ctx, dtype, tab.data(), cfgs.data(), n, a.peak);
                break;
            }
            case VSZIP_STAGE_LIMITER: {
                const auto &a = params_of<vszip_chain_limiter>(op);
                std::vector<double> lo(n), hi(n);
                for (int k = 0; k < n; ++k) {
                    lo[k] = a.lo[plane_slot[steps[k].entry]];
                    hi[k] = a.hi[plane_slot[steps[k].entry]];
                }
                rc = vszip_limiter(ctx, dtype, tab.data(), n, lo.data(), hi.data());
                break;
            }
            case VSZIP_STAGE_CLAHE: {
                const auto &a = params_of<vszip_chain_clahe>(op);
                rc = vszip_clahe(ctx, dtype, tab.data(), n, a.limit, a.tiles_x, a.tiles_y);
                break;
            }
            case VSZIP_STAGE_COMB_MASK: {
                const auto &a = params_of<vszip_chain_comb_mask>(op);
                if (a.mthresh > 0)  // the previous frame of the slot, where the op before left it
                    for (int k = 0; k < n; ++k) place(steps[k].p1, steps[k].reads, &tab[k].ref, &tab[k].ref_stride);
                rc = vszip_comb_mask(ctx, tab.data(), n, a.cthresh, a.mthresh, a.expand, a.metric);
                break;
            }
            case VSZIP_STAGE_COMB_MASK_MT: {
                const auto &a = params_of<vszip_chain_comb_mask_mt>(op);
                rc = vszip_comb_mask_mt(ctx, tab.data(), n, a.thy1, a.thy2);
                break;
            }
            case VSZIP_STAGE_CHECKMATE: {
                const auto &a = params_of<vszip_chain_checkmate>(op);
                std::vector<vszip_temporal_nbrs> nb(n);
                for (int k = 0; k < n; ++k) {
                    const cp::Step &st = steps[k];
                    place(st.p2, st.reads, &nb[k].p2, &nb[k].p2_stride);
                    place(st.p1, st.reads, &nb[k].p1, &nb[k].p1_stride);
                    place(st.n1, st.reads, &nb[k].n1, &nb[k].n1_stride);
                    place(st.n2, st.reads, &nb[k].n2, &nb[k].n2_stride);
                }
                rc = vszip_checkmate(ctx, tab.data(), nb.data(), n, a.thr, a.tmax, a.tthr2);
                break;
            }
            case VSZIP_STAGE_MOSQUITO_NR: {
                const auto &a = params_of<vszip_chain_mosquito_nr>(op);
                std::vector<int32_t> st, rs, rd;
                std::vector<uint8_t> ch;
                const int32_t *pst = gather(st, a.strength, steps), *prs = gather(rs, a.restore, steps), *prd = gather(rd, a.radius, steps);
                rc = vszip_mosquito_nr(ctx, dtype, bits_per_sample, tab.data(), n, pst, prs, prd, gather(ch, a.chroma, steps));
                break;
            }
            case VSZIP_STAGE_DEBAND: {
                const auto &a = params_of<vszip_chain_deband>(op);
                std::vector<vszip_deband_plane> per;
                rc = vszip_deband(ctx, dtype, tab.data(), gather(per, a.per, steps), n, a.sample_mode, a.blur_first, a.angle_boost, a.max_angle, a.max_offset);
                break;
            }
            case VSZIP_STAGE_BILATERAL_DITHER: {
                const auto &a = params_of<vszip_chain_bilateral_dither>(op);
                std::vector<vszip_bilateral_dither_plane> per;
                rc = vszip_bilateral_dither(ctx, dtype, bits_per_sample, tab.data(), gather(per, a.per, steps), n);
                break;
            }
            case VSZIP_STAGE_COMPRESS: {
                const auto &a = params_of<vszip_chain_compress>(op);
                std::vector<uint8_t> ch;
                rc = vszip_compress(ctx, tab.data(), n, a.tables, gather(ch, a.chroma, steps));
                break;
            }
            default:  // (the plan refused it)
                return vszip_set_error(ctx, VSZIP_ERR_ARG, "chain: op %d: kind %d", s, op.kind);
        }
        if (rc != VSZIP_OK) return rc;
    }
    // planes no op filters pass through
    for (int i : plan.copies)
        if (planes[i].dst != planes[i].src) {
            rc = vszip_copy_d2d_2d(ctx, planes[i].dst, (size_t)planes[i].dst_stride * bps, planes[i].src, (size_t)planes[i].src_stride * bps, (size_t)planes[i].w * bps, (size_t)planes[i].h);
            if (rc != VSZIP_OK) return rc;
        }
    return VSZIP_OK;
}

// the three kinds of the flat stage struct, as ops
VSZIP_EXPORT int vszip_chain_run(vszip_ctx *ctx, int dtype, const vszip_chain_stage *stages, int nstages, const vszip_plane *planes, const int *plane_slot, int nplanes) {
    if (!ctx || !stages || !planes || !plane_slot || nstages <= 0 || nplanes <= 0) return VSZIP_ERR_ARG;
    std::vector<vszip_chain_op> ops(nstages);
    std::vector<vszip_chain_boxblur> bb(nstages);
    std::vector<vszip_chain_bilateral> bl(nstages);
    std::vector<vszip_chain_limiter> lm(nstages);
    for (int s = 0; s < nstages; ++s) {
        const vszip_chain_stage &st = stages[s];
        ops[s].kind = st.kind;
        for (int k = 0; k < 3; ++k) ops[s].process[k] = st.process[k];
        bb[s] = {st.hradius, st.hpasses, st.vradius, st.vpasses};
        bl[s] = {{st.bilateral[0], st.bilateral[1], st.bilateral[2]}, st.peak};
        for (int k = 0; k < 3; ++k) lm[s].lo[k] = st.lo[k], lm[s].hi[k] = st.hi[k];
        ops[s].params = st.kind == VSZIP_STAGE_BOXBLUR ? (const void *)&bb[s] : st.kind == VSZIP_STAGE_BILATERAL ? (const void *)&bl[s] : (const void *)&lm[s];
        if (st.kind < VSZIP_STAGE_BOXBLUR || st.kind > VSZIP_STAGE_LIMITER) return vszip_set_error(ctx, VSZIP_ERR_ARG, "chain: stage kind %d", st.kind);  // (the flat struct has no fields for the newer kinds)
    }
    return vszip_chain_ops(ctx, dtype, 0, ops.data(), nstages, planes, plane_slot, nullptr, nplanes);
}
