/*
 * vszip_hip.h — flat C ABI of the MI355X (gfx950) vszip pixel kernels.
 *
 * This is the drop-in boundary: the cut between the reference's filter wrappers
 * (src/vapoursynth/NAME.zig, layer L2) and its pixel kernels (src/filters/NAME.zig,
 * layer L3).  Every entry point replaces one L3 function the wrappers call, takes
 * plain pointers, strides IN ELEMENTS (as ZAPI getDimensions2 returns them,
 * src/vapoursynth/boxblur.zig:46) and scalars, and returns 0 or a negative
 * vszip_status.  No C++ / HIP / torch types appear in any signature; a Zig host
 * binds it with `extern "c"` declarations.
 *
 * All plane pointers are DEVICE pointers (hipMalloc, or any allocator that
 * yields device-accessible memory, e.g. a torch CUDA tensor's data_ptr).  Host
 * VSFrame planes are staged with vszip_copy_h2d_2d / vszip_copy_d2h_2d on the
 * context's stream.  Kernels are enqueued on the context's stream and return
 * without synchronising unless stated (the metric filters copy their scalars
 * back and synchronise, because their result is a host scalar).
 */
#ifndef VSZIP_HIP_H
#define VSZIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSZIP_ABI_VERSION 4 /* additive since 4: vszip_clahe, vszip_comb_mask, vszip_comb_mask_mt, vszip_checkmate, vszip_mosquito_nr, vszip_deband, vszip_deband_tables, vszip_bilateral_dither, vszip_bilateral_dither_derive, vszip_bilateral_dither_points, vszip_compress, vszip_compress_tables, vszip_pack_rgb, vszip_color_map_lut, vszip_color_map, vszip_image_unpack, vszip_chain_ops; 4 (round 5): vszip_dev_alloc searches a bounded number of candidates and keeps nothing (below); vszip_dev_arena_info added; vszip_dev_trim, vszip_dev_placement_info and
                               vszip_dev_alloc_probed removed (nothing is searched for or parked any more); 3 (round 4): vszip_ctx_set_option / _get_option, vszip_dev_probe_region,
                               vszip_plane_average_async, vszip_plane_minmax_async added; 2 (round 3): vszip_ssim_source grew (YUV sources); entry points added since 1:
                               vszip_chain_run, vszip_ssimulacra2_src, vszip_to_rgbs_linear, vszip_probe_read_each, vszip_resample_table */

typedef struct vszip_ctx vszip_ctx;

/* sample types: helper.zig:59-108 DataType. U32 is accepted by vszip_plane_average and vszip_limiter only, like in
 * the reference (enable_u32, helper.zig:78), and without an exclude list (planeaverage.zig(vs):127). */
enum vszip_dtype { VSZIP_U8 = 0, VSZIP_U16 = 1, VSZIP_F16 = 2, VSZIP_F32 = 3, VSZIP_U32 = 4 };

enum vszip_status {
    VSZIP_OK = 0,
    VSZIP_ERR_ARG = -1,         /* invalid argument (the wrapper's create-time checks) */
    VSZIP_ERR_HIP = -2,         /* a HIP runtime call failed; see vszip_last_error */
    VSZIP_ERR_UNSUPPORTED = -3, /* valid in the reference, not built yet (DESIGN.md section 1 lists the cases) */
    VSZIP_ERR_NOMEM = -4
};

/* ---- context: one per (process, GPU); owns a stream and scratch ---------- */
int vszip_ctx_create(int device, vszip_ctx **out);
void vszip_ctx_destroy(vszip_ctx *ctx);
/* Use an externally owned hipStream_t (passed as void*) instead of the context's own; NULL is the null stream. Hand-over: everything
 * the context queues on the new stream is ordered after everything it queued on its previous stream (the context's scratch, scalar
 * buffers and tables are shared by consecutive calls) - the own stream is drained and destroyed, a caller's previous stream is joined
 * with an event, so that stream must still exist at the time of this call. Work the CALLER queued on either stream is not ordered. */
int vszip_ctx_set_stream(vszip_ctx *ctx, void *hip_stream);
void *vszip_ctx_stream(vszip_ctx *ctx);
int vszip_ctx_sync(vszip_ctx *ctx);
/* How vszip_copy_h2d_2d / _d2h_2d move host memory. 0 (default): straight from/to the caller's pointers
 * (right for pinned memory; pageable memory is pinned in place by the runtime, one copy at a time
 * per process). 1: through the context's own pinned arena with CPU copies — the DMA is asynchronous
 * and concurrent across contexts, D2H data reaches the caller's memory inside vszip_ctx_sync.
 * Env VSZIP_STAGING=pinned selects 1 for every new context. */
int vszip_ctx_set_staging(vszip_ctx *ctx, int mode);
/* Options. Every switch of the library (vapoursynth-zip_amd/csrc/options.inc lists them with their defaults) is read from the
 * environment ONCE, when the context is created, under the name given here (e.g. "VSZIP_PLACEMENT", "VSZIP_STAGING",
 * "VSZIP_RT_NO_ICHAIN"); these two change / read one on a live context. Flags are 0 / 1. VSZIP_ERR_ARG: no such option;
 * VSZIP_ERR_UNSUPPORTED: a development variant that this build does not contain (-DVSZIP_DEV_VARIANTS).
 * Read-only counters (get only): "VSZIP_STAT_MINMAX_PREDICTED", "VSZIP_STAT_MINMAX_FALLBACKS", "VSZIP_STAT_SCRATCH_KIB" (the context's scratch buffer, KiB). */
int vszip_ctx_set_option(vszip_ctx *ctx, const char *name, int value);
int vszip_ctx_get_option(vszip_ctx *ctx, const char *name, int *value);
/* Error path of a caller that gives up on the current frame: drains the stream and forgets staged
 * D2H copies that have not reached their destination yet (the destinations may then be freed). */
int vszip_ctx_abort(vszip_ctx *ctx);
const char *vszip_last_error(vszip_ctx *ctx);
int vszip_abi_version(void);

/* ---- device memory + staging (replaces nothing: the reference is host-only) */
/* vszip_dev_alloc. Requests of VSZIP_PLACEMENT_MIN_MIB (256) or more are PLACED: kernels with thousands of concurrent row
 * streams (the BoxBlur ring kernels) run 15-20 % slower with their destination planes in most physical memory than in some,
 * a stable property of the allocation that nothing user space can see predicts (profiles/r05_placement.md). Up
 * to VSZIP_PLACEMENT_TRIES (24) candidate allocations of the requested size are made (all held meanwhile, so each lies
 * elsewhere; never more than a quarter of what hipMemGetInfo reports free), each classified with a 2 ms copy in the ring
 * kernels' access shape; the search ends with the first candidate of the best class, else the fastest is kept, and every other
 * candidate is freed before the call returns (a few milliseconds per candidate; more where the driver clears memory that was
 * used before). The search is bounded: no candidate is started after VSZIP_PLACEMENT_BUDGET_MS (300) of wall clock; it ends early
 * at a candidate within 1.5 % of the best probe rate this process has seen on the device (a device's first search: at the
 * calibrated best class); and a device whose searches found all candidates alike twice in a row (one class of memory, or too
 * busy to measure) is served with plain hipMalloc from then on. No memory is cached or parked; the only state is that per-device
 * record (best rate seen, verdict). vszip_dev_free is hipFree.
 * VSZIP_PLACEMENT=0 (or vszip_ctx_set_option): plain hipMalloc. */
int vszip_dev_alloc(vszip_ctx *ctx, size_t bytes, void **dptr);
/* What the search did for `dptr` (as returned by vszip_dev_alloc); any pointer may be NULL. *candidates = 0: a plain allocation;
 * *probe_bytes_per_second: the classification copy's rate on the one kept (0: one candidate, not probed). */
int vszip_dev_arena_info(vszip_ctx *ctx, const void *dptr, int *candidates, double *probe_bytes_per_second, double *search_ms);
/* Diagnostic: a copy in the ring kernels' access shape on a caller's region (overwrites its contents): bytes / s. `from` == NULL: tiles
 * are read and written inside the region; else they are read from `from` (another region of at least `bytes`, not modified). */
int vszip_dev_probe_region(vszip_ctx *ctx, void *dptr, size_t bytes, const void *from, double *bytes_per_second);
/* any context of the process may free any allocation of that device; NULL is accepted */
int vszip_dev_free(vszip_ctx *ctx, void *dptr);
int vszip_dev_memset(vszip_ctx *ctx, void *dptr, int value, size_t bytes);
int vszip_host_alloc_pinned(vszip_ctx *ctx, size_t bytes, void **hptr);
int vszip_host_free_pinned(vszip_ctx *ctx, void *hptr);
/* pitches in BYTES; async on the context stream: a copy is complete when vszip_ctx_sync returns */
int vszip_copy_h2d_2d(vszip_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t rows);
int vszip_copy_d2h_2d(vszip_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t rows);
int vszip_copy_d2d_2d(vszip_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t rows);

/* ---- timing helpers (HIP events on the context stream; used by bench.py) -- */
int vszip_timer_start(vszip_ctx *ctx);
int vszip_timer_stop_ms(vszip_ctx *ctx, float *ms); /* synchronises */
/* Dominant-kernel probe: while enabled, every filter call brackets the launch of its dominant
 * kernel (BoxBlur: the CT ring kernel; Bilateral: the truncated-window kernel; SSIMULACRA2: the
 * per-scale maps kernel) with HIP events on the context's stream. vszip_probe_read synchronises,
 * returns the summed kernel time and the number of launches, and resets the probe. Measurement
 * aid for bench.py's roofline (the figure rocprofv3 --kernel-trace reports per kernel). */
int vszip_probe_enable(vszip_ctx *ctx, int on);
int vszip_probe_read(vszip_ctx *ctx, double *total_ms, int *launches);
/* the same, also copying the first `cap` launch durations (ms, launch order) to each_ms */
int vszip_probe_read_each(vszip_ctx *ctx, double *total_ms, int *launches, float *each_ms, int cap);

/* One plane of one frame. Strides in elements of the sample type.
 *
 * Plane memory: what a call reads and writes. Valid for every entry point that takes planes: the vszip_plane table calls
 * and the pointer-array calls (vszip_ssimulacra2 / _src, vszip_to_rgbs_linear, vszip_xpsnr_wsse / _batch, the sclips /
 * mclips of vszip_eedi3 / _mclip, vszip_limit_filter's refs, vszip_adaptive_binarize's second clip, vszip_comb_mask's
 * previous frame in `ref`, the tables and grain of vszip_deband's vszip_deband_plane and the neighbouring frames' planes of vszip_checkmate's vszip_temporal_nbrs, which are inputs
 * under clauses 1-3 with the size of the entry's plane and pitches of their own: h x stride readable each). A plane is
 * (pointer, stride, w, h) with stride >= w. Derived from the kernels ("Furthest read of every
 * kernel") and kept by tests/test_gpu_footprint.py.
 *
 * 1. Readable extent. For every INPUT plane the caller provides h x stride samples of mapped device memory from the
 *    plane pointer: the pitch padding [w, stride) of every row, the last row's included. Vector paths load whole
 *    16-byte lane groups and may read padding (never beyond h x stride; what they read there is masked out, clause 2).
 *    Nothing before the plane pointer is read. For every OUTPUT plane the caller owns h x stride samples likewise (the
 *    ring kernels' store descriptors are bounded by that product), although only clause 3's samples are written.
 * 2. Independence. No output sample, returned scalar or error code depends on any byte outside [0, w) x h of the input
 *    planes: not on pitch padding, not on memory between or around planes. Inside [0, w) x h every sample is an input,
 *    with one exception: vszip_eedi3 / _mclip with dh = 0 and horizontal = 0 never read the source rows of parity `field`
 *    (those are the rows the call interpolates; planes[i].src has the full height h, of which rows field, field + 2, ...
 *    may hold anything).
 * 3. Written extent. Input planes are never written. Of an output plane a call writes [0, w) of each of its h rows and
 *    nothing else: no pitch padding, no byte before the plane, none after column w - 1 of row h - 1. This holds on
 *    every path, the 16-byte vector paths included (their last lane group is masked or finished by scalar stores); a
 *    window into a larger picture keeps its neighbours.
 * 4. Base alignment and aliasing. Every base alignment of the sample type and every stride >= w are accepted. The fast
 *    paths need plane pointers and row pitches (in bytes) that are multiples of 16 (what hipMalloc and VapourSynth
 *    frames give); anything else takes a slower kernel with the same results, bit for bit. One combination is refused
 *    instead of served: a horizontal pass of vszip_boxblur's run-time-radius integer path over rows longer than 16000
 *    samples needs 16-byte aligned planes (VSZIP_ERR_UNSUPPORTED). Nothing is ever silently wrong for an alignment.
 *    dst == src (same pointer, same stride) is allowed for the point filters vszip_limiter, vszip_limit_filter (dst may
 *    be the flt plane, the source plane or refs[i]) and vszip_adaptive_binarize (dst may be either clip), whose every
 *    output sample depends on the input samples at the same position only, and for vszip_clahe (the histograms are
 *    complete before the first store). Every other filter reads neighbourhoods: dst must not overlap any input, and
 *    two output planes of one call must not overlap each other; vszip_comb_mask and vszip_comb_mask_mt are of this kind
 *    (rows above and below, and the previous frame's plane in `ref`): their dst must overlap neither src nor ref, while
 *    ref may be the very src pointer. vszip_checkmate likewise: any of its four neighbour planes may be the very src pointer
 *    or each other (what clamping frame indices to the clip produces at its ends), dst must overlap no input, and only
 *    [0, w) x h of dst is written (the reference copies two whole pitches at either end of a plane, padding included; this
 *    library does not). vszip_mosquito_nr reads a 9 x 9 neighbourhood: clauses 1-4 hold, its dst must not overlap src (for a
 *    plane with strength 0, which is copied, too), bases and pitches that are not multiples of four samples take a slower
 *    path with the same bits, and integer samples above 2^bits - 1 are not an error: they are processed as the reference
 *    would process them and the result is clamped to 2^bits - 1. vszip_deband reads two or four samples at per-sample offsets of up to
 *    128 samples in both directions, always inside [0, w) x h (every sampled coordinate is clamped, whatever the table holds): clauses 1-4 hold,
 *    its dst must not overlap src, only [0, w) x h of dst is written, and bases and pitches that are not multiples of four samples take a
 *    slower path with the same bits. Its offset tables and grain planes (vszip_deband_plane) are inputs under clauses 1-3 with the size of
 *    the entry's plane and pitches of their own: h x offsets_pitch pairs and h x grain_pitch samples readable each; no output depends on their
 *    padding either. vszip_bilateral_dither reads a (2 radius - 1)^2 window mirrored at the plane's edges: its reads stay inside
 *    [0, w) x h of src and ref, the whole point table (23 x K pairs) is an input, only [0, w) x h of dst is written, dst must overlap no
 *    input, ref may be the very src pointer, and every base alignment and pitch takes the same path. vszip_compress works on 8 x 8
 *    blocks with no neighbourhood: its reads stay inside [0, w) x h of src (a partial block at the right or bottom edge replicates the
 *    last in-plane column or row, min(x, w - 1) / min(y, h - 1), and never reads pitch padding), only [0, w) x h of dst is written,
 *    and dst == src (same pointer, same stride) is allowed, because a block reads and writes only its own 8 x 8 samples and is read
 *    completely before it is stored; any other overlap is not allowed. Every base alignment and pitch is served: a fast path for
 *    bases and pitches that are multiples of 8 bytes, and a slower one with the same bits. Partial overlap is never allowed.
 *    vszip_pack_rgb and vszip_color_map are point filters whose planes differ in number and sample width (three planes in and one
 *    32-bit plane out; one plane in and three out): their reads stay inside [0, w) x h of every input (pitch padding is never read),
 *    only [0, w) x h of every output is written, r, g and b of vszip_pack_rgb may be the very same pointer or overlap each other,
 *    no output may overlap an input, and the three outputs of vszip_color_map must not overlap each other. Every base alignment of
 *    the sample type and every pitch >= w is served: a fast path for bases and pitches (in bytes) that are multiples of 16 on every
 *    plane of the frame, and a slower one with the same bits. vszip_image_unpack is the mirror of vszip_pack_rgb, one packed buffer in
 *    and up to four planes out: its reads stay inside the w x pixel-bytes of each of the h source rows (the source's pitch is in bytes
 *    and its padding is never read), only [0, w) x h of each output plane is written, and the outputs overlap neither each other nor
 *    src. The source needs no alignment at all; frames whose output bases and pitches (in bytes) are multiples of 16 take the fast
 *    path, every other frame a slower one with the same bits. vszip_depth converts one plane into one plane of another sample width:
 *    its reads stay inside [0, w) x h of src, only [0, w) x h of dst is written, dst overlaps no src, and bases and pitches (in
 *    bytes) that are not multiples of 16 take per-sample accesses with the same bits. vszip_deband_lowbit is vszip_deband's clauses
 *    on planes of the lower depth.
 */
typedef struct vszip_plane {
    const void *src; /* input plane */
    void *dst;       /* output plane (filters that write pixels) */
    const void *ref; /* second input: Bilateral `ref`, PlaneAverage/MinMax `clipb`; NULL if none */
    ptrdiff_t src_stride;
    ptrdiff_t dst_stride;
    ptrdiff_t ref_stride;
    int32_t w;
    int32_t h;
} vszip_plane;

/*
 * BoxBlur — replaces boxblur_ct.hvBlur (src/filters/boxblur_comptime.zig:10) and
 * the RT chain hblur / vblur / hvBlurFused (src/filters/boxblur_runtime.zig:121,
 * 153, 283) as dispatched by src/vapoursynth/boxblur.zig:85-113,188-209.
 * Processes `nplanes` independent planes (any mix of sizes, e.g. Y,U,V of many
 * frames) in one call; path choice (CT vs RT) follows boxblur.zig:188.
 * Errors mirror boxBlurCreate (boxblur.zig:150-179): nothing to be performed,
 * 2*radius >= plane size -> VSZIP_ERR_ARG.
 */
int vszip_boxblur(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes,
                  int hradius, int hpasses, int vradius, int vpasses);

/*
 * PlaneAverage — replaces filter.average / filter.averageRef
 * (src/filters/planeaverage.zig:26,47) called from src/vapoursynth/planeaverage.zig:55-61.
 * planes[i].ref != NULL on plane 0 selects the clipb variant for all planes.
 * `exclude` is the i32 list of the wrapper (:122-137; compared as @floatFromInt for
 * float clips), any length (up to 256 distinct values). bits_per_sample gives peak = 2^bits - 1 (:115).
 * Results are written to host arrays avg[nplanes] and (clipb) diff[nplanes]; the call
 * synchronises the stream. Integer planes are exact; float planes differ from the
 * reference's sequential f64 sum by rounding only.
 */
int vszip_plane_average(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes,
                        const int32_t *exclude, int nexclude, int bits_per_sample,
                        double *avg, double *diff);
/* The same without the synchronise (round 4): the per-plane results are written by the kernels straight into the caller's PINNED
 * host array `pinned_results` (vszip_host_alloc_pinned; nplanes x 4 doubles: [i][0] = avg, [i][1] = diff for the clipb variant)
 * and are valid after the caller's next vszip_ctx_sync — a host that reads several statistics of a frame queues them all and
 * waits once. */
int vszip_plane_average_async(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes,
                              const int32_t *exclude, int nexclude, int bits_per_sample, double *pinned_results);

/*
 * Limiter — replaces the getFrame bodies of LimiterRT / Limiter (src/vapoursynth/limiter.zig:28-96):
 * dst = min(max(lo, x), hi) in the sample type, per plane. lo[i] / hi[i] are the bounds the wrapper
 * resolved for planes[i] — the min/max arrays (u32 for integer clips, f32 for float clips), or the
 * comptime range tables of src/filters/limiter.zig:66-91 (full / tv_range yuv / rgb per depth,
 * yuvf / rgbf). dtype may be VSZIP_U32. Asynchronous on the context stream.
 */
int vszip_limiter(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes, const double *lo,
                  const double *hi);

/*
 * LimitFilter — replaces filter.process (src/filters/limit_filter.zig:3-34) called from
 * LimitFilter(T, refb).getFrame (src/vapoursynth/limit_filter.zig:27-80). planes[i].src is the
 * FILTERED clip's plane (`flt`), planes[i].ref the SOURCE clip's (`src`), planes[i].dst the output;
 * refs[i] (may be NULL, as may the array) is the optional third clip the difference is taken
 * against (default: the source), strides in elements. dark_thr / bright_thr are on the clip's own
 * scale (the wrapper applies hz.scaleValue, src/helper.zig:312-336, to the 8-bit-scale arguments),
 * elast as given; one value per plane. Asynchronous on the context stream.
 */
int vszip_limit_filter(vszip_ctx *ctx, int dtype, const vszip_plane *planes, const void *const *refs,
                       const ptrdiff_t *ref_strides, int nplanes, const float *dark_thr,
                       const float *bright_thr, const float *elast);

/*
 * AdaptiveBinarize — replaces the getFrame body of src/vapoursynth/adaptive_binarize.zig:26-73:
 * 8-bit planes, dst = 255 where clip2 - clip >= c (compared in i16, c clamped to [-256, 256]
 * :96-99), else 0. planes[i].src is `clip`'s plane, planes[i].ref `clip2`'s. Asynchronous.
 */
int vszip_adaptive_binarize(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, int c);

/*
 * CLAHE — replaces filter.applyCLAHE (src/filters/clahe.zig:14-38: calcLut :40-156, interpolate :176-282) as called per plane by
 * CLAHE(T).getFrame (src/vapoursynth/clahe.zig:23-49). dtype VSZIP_U8 or VSZIP_U16; every plane equalised with its own size; dst may equal src.
 * Asynchronous on the context stream.
 * Any number of planes of any sizes (the planes of many frames) in one call; `limit` and tiles_x / tiles_y are the wrapper's
 * d.limit and d.tiles. VSZIP_ERR_ARG, each with its own vszip_last_error text, for the wrapper's create-time checks
 * (clahe.zig(vs):70-112) applied to every plane of the table: a dtype other than U8 / U16, tiles_x or tiles_y < 1, a tile
 * count above a plane's width or height, limit * tile area / hist_size above INT32_MAX. Histograms and LUTs live in the
 * context's scratch (grow-only), at most VSZIP_CLAHE_SCRATCH_MIB of it per plane group (csrc/options.inc).
 */
int vszip_clahe(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes, uint32_t limit, int tiles_x, int tiles_y);

/*
 * CombMask — replaces filter.process (src/filters/comb_mask.zig:18-47: metric0Mask :49, metric1Mask :101, motionMaskAnd :142,
 * expandMask :180) as called per plane by CombMask(metric_1, expand, motion).getFrame (src/vapoursynth/comb_mask.zig:22-61).
 * 8-bit planes, each with its own size (h >= 3). planes[i].src is the plane of frame n, planes[i].dst the mask (255 / 0);
 * planes[i].ref is the same plane of frame max(0, n - 1): required when mthresh > 0 (it may be the very src pointer, as for
 * frame 0: the mask is then all zero), ignored when mthresh == 0. cthresh, mthresh, expand, metric are the wrapper's arguments
 * (defaults 6, 9, 1, 0). One fused pass: no intermediate plane, no scratch. Asynchronous on the context stream.
 * VSZIP_ERR_ARG, with the wrapper's create-time wording in vszip_last_error (comb_mask.zig(vs):93-120): cthresh outside
 * 0..255 (metric 0) or 0..65025 (metric 1), mthresh outside 0..255, a plane with fewer than 3 rows; and a NULL src or dst,
 * or a NULL ref with mthresh > 0. Only [0, w) x h of dst is written ("Plane memory"; the reference also writes pitch padding).
 */
int vszip_comb_mask(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, int cthresh, int mthresh, int expand, int metric);

/*
 * CombMaskMT — replaces filter.process (src/filters/comb_mask_mt.zig:11-66) as called per plane by CombMaskMT(same_thr).getFrame
 * (src/vapoursynth/comb_mask_mt.zig:22-59). 8-bit planes (h >= 3): rows 0 and h - 1 are 0; elsewhere p = (up - s) * (down - s)
 * gives 255 where p > thY2, 0 where p < thY1 (thY1 == thY2: where p <= thY2) and min((p - thY1) * 256 / (thY2 - thY1), 255) in
 * between. `ref` is not used. Asynchronous. VSZIP_ERR_ARG with the wrapper's wording (comb_mask_mt.zig(vs):87-110): thY1 or thY2
 * outside [0;255], thY1 > thY2, a plane with fewer than 3 rows; and a NULL src or dst.
 */
int vszip_comb_mask_mt(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, int thy1, int thy2);

/*
 * Checkmate — replaces filter.process (src/filters/checkmate.zig:5-57) and the row loop around it in Checkmate(use_tthr2).getFrame
 * (src/vapoursynth/checkmate.zig:26-96). The first filter here whose frame n reads up to five frames: planes[i].src is the plane
 * of frame n, planes[i].dst the output (`ref` is not used), and nbrs[i] names the same plane of frames n - 2 .. n + 2, each
 * with its own pitch, the frame indices already clamped to the clip as getFrame does (max(0, n - k), min(n + k, frames - 1)):
 * at a clip's ends they are the src pointer itself or each other. p2 and n2 are read only when tthr2 > 0 and may be NULL
 * otherwise. 8-bit planes, each with its own size (w >= 3, h >= 5), so the planes of a whole clip fit in one call with the
 * clip's own frames as each other's neighbours. Rows 0, 1, h - 2, h - 1 are copies of src; elsewhere the output blends the
 * sample with a sharpened version of itself (rows y - 2, y, y + 2, columns x - 2, x, x + 2 clamped to the plane) and with frames
 * n - 1 and n + 1, weighted by how little the column sums differ (thr, tmax; defaults 12, 12), or, with tthr2 > 0 (default 0)
 * and all of |p1 - n1|, |p2 - src|, |src - n2| below tthr2, is (p1 + 2 src + n1) >> 2. One fused pass: no intermediate plane, no
 * scratch. Asynchronous on the context stream. VSZIP_ERR_ARG, with the wrapper's create-time wording in vszip_last_error
 * (checkmate.zig(vs):125-153, in its order): tmax outside [1;255], tthr2 negative, thr outside [0;255], a plane narrower than 3
 * or shorter than 5; and a NULL src, dst, p1 or n1, or a NULL p2 or n2 with tthr2 > 0.
 */
typedef struct vszip_temporal_nbrs { /* the same plane of the neighbouring frames, already clamped to the clip by the caller */
    const void *p2, *p1, *n1, *n2;   /* frames n-2, n-1, n+1, n+2; p2 / n2 ignored (may be NULL) when the filter does not use them */
    ptrdiff_t p2_stride, p1_stride, n1_stride, n2_stride;
} vszip_temporal_nbrs;

int vszip_checkmate(vszip_ctx *ctx, const vszip_plane *planes, const vszip_temporal_nbrs *nbrs, int nplanes,
                    int thr, int tmax, int tthr2);

/*
 * MosquitoNR — replaces MosquitoNR(T).process (src/filters/mosquito_nr.zig:264-386: the padding :297-326, smooth :31-162, fwdV / fwdH /
 * invH / invV :164-262, the LL mix :353-360, the store :366-385) and MosquitoNRFloat.process (src/filters/mosquito_nr_float.zig:263-369)
 * as called per plane by Filter(T).getFrame (src/vapoursynth/mosquito_nr.zig:30-82). dtype VSZIP_U8 (bits_per_sample 8), VSZIP_U16
 * (9..16) or VSZIP_F32 (bits_per_sample is ignored); one dtype per call, any number of planes of any sizes (at least 4 x 4), so the
 * planes of many frames fit in one call. strength[i] (0..32; the wrapper's default 16), restore[i] (0..128; 128) and radius[i] (1 or
 * 2; 2) belong to planes[i]; chroma[i] != 0 clamps a float plane to [-0.5, 0.5] instead of [0, 1] (the wrapper passes plane > 0), NULL
 * means all luma, and it is ignored for integers. `ref` is not used. A plane with strength 0 is copied ([0, w) x h only). One fused
 * pass: the nine passes and eleven scratch planes of the reference happen in LDS, tile by tile; no scratch. Bit-exact with the
 * reference in all three sample types, float included. Asynchronous on the context stream. VSZIP_ERR_ARG, with the wrapper's wording in
 * vszip_last_error (mosquito_nr.zig(vs):99-134, in its order): a dtype / bits_per_sample combination outside the list, a plane narrower
 * or shorter than 4, and strength, restore or radius out of range with hz.getArray's texts ("MosquitoNR: strength value 33 is above
 * maximum 32."); and a NULL parameter array, src or dst.
 */
int vszip_mosquito_nr(vszip_ctx *ctx, int dtype, int bits_per_sample, const vszip_plane *planes, int nplanes,
                      const int32_t *strength, const int32_t *restore, const int32_t *radius, const uint8_t *chroma);

/*
 * Deband — f3kdb-style debanding with grain: replaces processPlane of src/filters/deband_int.zig:93-340 and
 * src/filters/deband_float.zig:88-309 (with fillAnglePlane / calculateGradientAngle and the polynomial pow / atan of src/vcl.zig)
 * as called per plane by F3KDB(...).getFrame, and the create-time tables of TempBuff.initFrameLuts
 * (src/vapoursynth/deband.zig:162-319, generators :336-431).
 *
 * vszip_deband_tables (device-free). Fills caller-provided HOST arrays for one clip geometry; with luma == NULL it only fills
 * `sizes` (the query). Outputs:
 *   luma, chroma   int8 pairs (val1, val2), one pair per plane sample, row pitch = the plane's width in pairs (chroma:
 *                  sizes.chroma_w x sizes.chroma_h = the luma size divided by 2^ssw x 2^ssh, rounded up); val2 = 0 outside
 *                  sample mode 2. These are the refEncode()d values themselves (0..127, or -128 where the reference's signed
 *                  char wraps), not multiplied by any pitch; the chroma entry at (cx, cy) is the luma entry at
 *                  (cx << ssw, cy << ssh) and the kernel applies the arithmetic >> ssw / >> ssh;
 *   grain_y/_c     sizes.grain_items values each (((width + 255) & ~127) * height, times 3 for dynamic grain), int16 for
 *                  integer clips and f32 for float clips; NULL (or strength 0) skips the buffer, its random values are
 *                  consumed all the same;
 *   grain_offsets  dynamic grain: one offset into both grain buffers per frame, (items + uniform(items)) & ~15;
 *   max_offset     the largest |val| in the tables (what vszip_deband wants to know).
 * grain_u16 / grain_f32 are the strengths on the clip's scale (what Data.scaleValue makes of the 8-bit-scale `grain`).
 * VSZIP_ERR_ARG with the reference's create-time wording in `err` (may be NULL) for the range checks of Data.setData that
 * concern these inputs, in its order: sample_mode [1..7], range [0..255], random_param_ref / _grain [0..255],
 * random_algo_ref / _grain [0..2] ('Deband: parameter "range=256" out of range [0..255].'). The checks of thr, thr1, thr2 and
 * grain are on the wrapper's 8-bit scale and stay with the host; angle_boost and max_angle are checked by vszip_deband.
 *
 * vszip_deband. dtype VSZIP_U16 (samples on the 16-bit scale: the reference always works at 16 bits; clips under 16 bits go
 * through vszip_deband_lowbit below, which converts up, runs these kernels and dithers back on the device) or VSZIP_F32. planes[i].src / dst as everywhere (`ref` is
 * not used); per[i] sits beside planes[i] as vszip_temporal_nbrs does:
 *   offsets, offsets_pitch  DEVICE pointer to the plane's table (luma or chroma) and its row pitch in pairs;
 *   ssw, ssh                the shifts to apply to the table's values (0 for luma);
 *   grain, grain_pitch      DEVICE pointer to the plane's grain (int16 for VSZIP_U16, f32 for VSZIP_F32), already advanced by
 *                           the frame's grain offset, and the pitch in samples the reference indexes it with (VapourSynth's
 *                           row pitch of the plane: the width rounded up to 32 bytes for the reference's goldens). It is
 *                           independent of the pitches of the planes given here. NULL: no grain;
 *   thr, thr1, thr2         on the clip's scale (integral values for VSZIP_U16); lo, hi: the output clamp.
 * Any number of planes of any sizes in one call; the planes of many frames share the same table pointers. sample_mode 1..7,
 * blur_first, angle_boost and max_angle are the wrapper's arguments; max_offset is the largest |val| of the tables used
 * (0..128). Entries beyond max_offset give an unspecified sample and no out-of-plane access: every sampled coordinate is
 * clamped, into the plane or into the tile a workgroup staged (for tables from vszip_deband_tables the clamp never changes
 * a coordinate). Two gather paths: a workgroup stages its tile and a halo of 32 samples in LDS (max_offset <= 32), or
 * gathers from global memory (any max_offset); VSZIP_DEBAND_PATH (csrc/options.inc) forces one. Sample mode 7 first writes the
 * normalised gradient angle of every plane into the context's scratch (grow-only; at most VSZIP_DEBAND_SCRATCH_MIB per
 * plane group, a plane is never split). Bit-exact with the reference in both sample types, float included. Asynchronous on
 * the context stream. "Plane memory": clauses 1-4 hold; only [0, w) x h of dst is written; dst must not overlap src;
 * bases and pitches (planes, table, grain) that are not multiples of four samples take a slower path with the same
 * bits; of a table (grain) plane h x offsets_pitch pairs (h x grain_pitch samples) must be readable. VSZIP_ERR_ARG with the
 * wrapper's wording for sample_mode, angle_boost [0..65535] and max_angle [0..1]; and for a dtype other than U16 / F32, a
 * max_offset outside 0..128, a NULL src, dst or table.
 */
typedef struct vszip_deband_cfg {
    int32_t width, height, ssw, ssh, num_frames; /* the clip: luma size, log2 chroma subsampling, frame count */
    int32_t range, sample_mode;
    int32_t seed, random_algo_ref, random_algo_grain; /* generators: 0 old, 1 uniform, 2 gaussian */
    double random_param_ref, random_param_grain;
    int32_t is_float, dynamic_grain;
    uint16_t grain_u16[2]; /* integer clips: luma, chroma strength on the 16-bit scale */
    float grain_f32[2];    /* float clips */
} vszip_deband_cfg;
typedef struct vszip_deband_sizes {
    size_t luma_pairs, chroma_pairs, grain_items, grain_offsets;
    int32_t chroma_w, chroma_h;
} vszip_deband_sizes;
typedef struct vszip_deband_plane {
    const int8_t *offsets;
    ptrdiff_t offsets_pitch;
    const void *grain;
    ptrdiff_t grain_pitch;
    int32_t ssw, ssh;
    float thr, thr1, thr2;
    float lo, hi;
} vszip_deband_plane;

int vszip_deband_tables(const vszip_deband_cfg *cfg, vszip_deband_sizes *sizes, int8_t *luma, int8_t *chroma, void *grain_y,
                        void *grain_c, uint32_t *grain_offsets, int32_t *max_offset, char *err, size_t err_cap);
int vszip_deband(vszip_ctx *ctx, int dtype, const vszip_plane *planes, const vszip_deband_plane *per, int nplanes,
                 int sample_mode, int blur_first, float angle_boost, float max_angle, int max_offset);

/*
 * Depth — integer depth conversion as zimg's resize.Point does it with dither_type none and error_diffusion: what hz.bitDepth
 * (src/helper.zig:470-494) asks the host's resizer for around Deband (src/vapoursynth/deband.zig:462-464, :494-497) and XPSNR. One
 * vszip_depth_plane per conversion: src a plane of bits_in, dst a plane of bits_out, 8 bits stored as uint8_t and 9..16 as uint16_t,
 * strides in elements of the plane's own sample type. Any number of planes of any mix of sizes in one call, w, h >= 1.
 *   scale   limited range: 2^(bits_out - bits_in). Full range, chroma 0 (RGB, gray, full-range luma): (2^bits_out - 1) / (2^bits_in - 1),
 *           divided in double and rounded to float. Full range with chroma set has a non-zero offset whose rounding no recorded data
 *           pins: VSZIP_ERR_UNSUPPORTED.
 *   dither 0 (none)             q = rint(min(max((float)src * scale, 0), 2^bits_out - 1)), half to even; one streaming pass.
 *   dither 1 (error diffusion)  Floyd-Steinberg in f32, rows top to bottom, samples left to right, every product and sum rounded on its
 *           own: err = 0 + left * 7/16; err += top[x + 1] * 3/16; err += top[x] * 5/16; err += top[x - 1] * 1/16;
 *           v = min(max(src * scale + err, 0), peak); q = rint(v); the sample's error is v - q; errors outside the plane are 0.
 *           Bit-exact with the reference's 8-bit Deband goldens (limited range 16 -> 8); the full-range case rests on this statement alone
 *           (DESIGN.md 3.18). One workgroup walks one plane as a skewed wavefront (csrc/depth_plan.hpp); a plane of more rows than a
 *           workgroup holds and more than 4096 columns keeps one row of errors in the context's scratch (grow-only).
 * Asynchronous on the context stream. "Plane memory": reads stay inside [0, w) x h of src; only [0, w) x h of dst is written; dst overlaps
 * no src. vszip_depth_check (device-free) is the argument check vszip_depth makes first, with the text in `err` (may be NULL):
 * VSZIP_ERR_ARG for bits_in or bits_out outside 8..16 ("Depth: bits_in 7 is outside 8..16"), a dither other than 0 or 1, no planes,
 * and, naming the plane ("Depth: plane 1: src and dst must not be NULL"), a NULL plane, w or h below 1, a pitch below w;
 * VSZIP_ERR_UNSUPPORTED for full-range chroma.
 *
 * vszip_deband_lowbit — vszip_deband on planes of `bits` = 8..15 (uint8_t for 8), as the wrapper runs Deband on clips under 16 bits:
 * per plane group, up to 16 bits with dither none, the kernels of vszip_deband, down to `bits` with error diffusion, on two 16-bit
 * intermediates per plane in the context's scratch (beside sample mode 7's angle planes; at most VSZIP_DEBAND_LOWBIT_SCRATCH_MIB of
 * intermediates per plane group, a plane is never split). per[i] stays on the 16-bit scale, exactly as vszip_deband takes it.
 * full_range 1 declares every plane non-chroma (RGB, gray); a full-range YUV clip's chroma is not served. Errors: vszip_deband's and
 * vszip_depth's, and VSZIP_ERR_ARG for bits outside 8..15.
 */
typedef struct vszip_depth_plane {
    const void *src;
    ptrdiff_t src_stride;
    void *dst;
    ptrdiff_t dst_stride;
    int32_t w, h;
    int32_t chroma; /* the plane is U or V of a YUV clip */
} vszip_depth_plane;
int vszip_depth_check(int bits_in, int bits_out, int dither, int full_range, const vszip_depth_plane *planes, int nplanes, char *err, size_t err_cap);
int vszip_depth(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, int bits_in, int bits_out, int dither, int full_range);
int vszip_deband_lowbit(vszip_ctx *ctx, int bits, int full_range, const vszip_plane *planes, const vszip_deband_plane *per, int nplanes,
                        int sample_mode, int blur_first, float angle_boost, float max_angle, int max_offset);

/*
 * DepthFmt — the change of sample type that resize.Point(format=...) makes on the host: between integer (VSZIP_U8 with bits 8, VSZIP_U16
 * with bits 9..16), half (VSZIP_F16, bits 16) and float (VSZIP_F32, bits 32) planes, as zimg does it (oracle/vs_host.py int_to_float /
 * float_to_int restate it; the reference's float and YUV goldens pass through those). What a caller with 8-bit frames needs around
 * vszip_eedi3 and the float paths of the other filters, and what the display path needs before vszip_pack_rgb. The plane struct is
 * vszip_depth_plane: src a plane of dtype_in, dst one of dtype_out, strides in elements of each plane's own sample type, `chroma` as for
 * vszip_depth. Any number of planes of any mix of sizes in one call, w, h >= 1. full_range describes the integer side; float <-> float
 * ignores it. IEEE f32 throughout. With
 *   limited range   off = (chroma ? 128 : 16) << (bits - 8),  rng = (chroma ? 224 : 219) << (bits - 8)
 *   full range      off = chroma ? 2^(bits - 1) : 0,          rng = 2^bits - 1
 *   int -> f32, dither 0    fmaf((float)v, f32(1.0 / rng), f32(-off / rng)): both constants divided in double and rounded once, ONE fused
 *           operation (the plain product when off is 0). All four range / chroma cases.
 *   f32 -> int, dither 0    q = rint(fmaf(x, (float)rng, (float)off)), half to even, clamped to [0, 2^bits - 1]. All four cases. +-Inf clamp;
 *           NaN is outside the contract.
 *   f32 -> int, dither 1    error diffusion where off is 0 (full range, chroma 0: RGBS, full-range gray or luma): vszip_depth's
 *           recurrence on src = the float sample with scale = (float)rng, the product rounded on its own. With an offset (limited range,
 *           or chroma) VSZIP_ERR_UNSUPPORTED: no recorded data pins whether zimg adds it fused (as for full-range chroma in vszip_depth).
 *   f16 -> f32 is exact; f32 -> f16 rounds to nearest even, subnormals kept, overflow to Inf.
 *   int <-> f16   as f32: the f32 result rounded to f16; the f16 sample widened, then the f32 rule. (No golden reaches half planes.)
 *   int -> int    vszip_depth itself, results and errors.
 * One streaming pass (a lane owns 16 bytes of the narrower plane), or vszip_depth's wavefront for the error diffusion, with its scratch
 * rule. Asynchronous on the context stream; "plane memory" as for vszip_depth: reads stay inside [0, w) x h of src, only [0, w) x h of
 * dst is written, dst overlaps no src. vszip_depth_fmt_check (device-free) is the argument check made first, text in `err` (may be NULL):
 * VSZIP_ERR_ARG for a dtype outside the four ("DepthFmt: dtype_in 4 is none of VSZIP_U8, VSZIP_U16, VSZIP_F16, VSZIP_F32"), bits that do
 * not fit the dtype ("DepthFmt: bits_in 8 does not fit VSZIP_U16 (9..16)"), a dither other than 0 or 1, dither 1 with a float destination
 * ("DepthFmt: error diffusion needs an integer destination, dtype_out is VSZIP_F32"), no planes, and, naming the plane, a NULL plane, w or
 * h below 1, a pitch below w; VSZIP_ERR_UNSUPPORTED for float -> integer error diffusion with an offset. Two integer dtypes: after the
 * dtype and bits checks, vszip_depth_check's codes and texts ("Depth: ...").
 */
int vszip_depth_fmt_check(int dtype_in, int bits_in, int dtype_out, int bits_out, int dither, int full_range, const vszip_depth_plane *planes,
                          int nplanes, char *err, size_t err_cap);
int vszip_depth_fmt(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, int dtype_in, int bits_in, int dtype_out, int bits_out,
                    int dither, int full_range);

/*
 * BilateralDither — the port of dither's Dither_bilateral16: replaces processPlane of src/filters/bilateral_dither.zig:34-213
 * as called per plane by GetFrame(T).gf (src/vapoursynth/bilateral_dither.zig:52-110), the per-plane derivation of its create
 * function (:151-209 with buildSlot :40-50) and generate of src/filters/bilateral_dither_subspl.zig:245-361.
 *
 * vszip_bilateral_dither_derive (device-free; replaces the derivation in create / buildSlot). One plane's wrapper arguments ->
 * m = max(thr scale, unit), wmax = max(thr (1 - flat) scale, unit), sum_w_min = max(wmin wmax N, unit) in f32 in the reference's
 * order (scale 2^(bits - 8) | 1/256, unit 1 | 1/65535 for integer | float clips; N = K sub-sampled, (2 radius - 1)^2 dense),
 * `subsampled` (subspl >= 4 or subspl < 1e-3) and K (0 for the dense window). VSZIP_ERR_ARG with hz.getArray's wording in
 * `err` (may be NULL) for radius [2..16384], thr [0..65535], flat [0..1], wmin [0..65535], subspl [0..4096]
 * ("BilateralDither: radius value 1 is below minimum 2."), and for integer bits outside 8..16.
 *
 * vszip_bilateral_dither_points (device-free; replaces subspl.generate with r_h == r_v == radius). Fills `points` (HOST memory,
 * `capacity` pairs, at least 23 K) with the 23 lists of K (x, y) int16 pairs, list after list; *K as derive gives it. points ==
 * NULL only returns K. Every list starts with (0, 0), holds no point twice and lies in [-(radius - 1), radius - 1]^2. The
 * void-and-cluster matrix of the lists with K >= 32 is built once a call.
 *
 * vszip_bilateral_dither. dtype VSZIP_U8 (bits_per_sample 8), VSZIP_U16 (9..16) or VSZIP_F32; planes[i].src / dst, and
 * planes[i].ref (optional, same size, its own pitch) as the plane that drives the weights; per_plane[i] beside planes[i]:
 *   radius            one radius per plane, as the reference's wrapper passes it (rh == rv), 2..16384, <= w and <= h;
 *   m, wmax, sum_w_min  from vszip_bilateral_dither_derive;
 *   points, K         DEVICE pointer to the 23 K pairs of vszip_bilateral_dither_points and K (3..4096): the sub-sampled path;
 *                     NULL and 0: the dense window.
 * Per output sample the taps are taken in the reference's order (dense: rows outer; sub-sampled: the points of list
 * (start(y) + (x >> 2)) % 23 in list order), each wgt = max(min(m - |vr - cen_ref|, wmax), 0), sum_w += wgt,
 * sum = fmaf(v - cen, wgt, sum); the result cen + sum / max(sum_w, sum_w_min) is clamped to [0, 2^bits - 1] and rounded half
 * away from zero for integers and stored as it is for float. Bit-exact with the reference in all three sample types. Two
 * paths: a workgroup stages its tile and a halo of radius - 1 samples, already mirrored, in LDS (and a second tile for
 * `ref`), or gathers from global memory with the mirror applied per tap (any radius); VSZIP_BILATERAL_DITHER_PATH
 * (csrc/options.inc) forces one, and a forced tile that does not fit takes the global path. A call is split into launches by
 * planes and row bands of a bounded number of taps each. Differences from the reference: the dense window serves radius <= 128
 * (VSZIP_ERR_UNSUPPORTED above; the sub-sampled path serves every radius), and the 16 x 16 minimum of the clip is the host's
 * check. VSZIP_ERR_ARG: 'BilateralDither: picture size must be greater than "radius"' for w or h below the radius, a radius
 * out of range, K > 0 without points (or points with K outside 3..4096), a NULL src or dst, a dst that is the src or ref pointer (any other overlap
 * is the caller's to avoid).
 * Asynchronous on the context stream. "Plane memory": reads stay inside [0, w) x h of src and ref; the whole point table is an
 * input; only [0, w) x h of dst is written.
 */
typedef struct vszip_bilateral_dither_cfg {
    float m, wmax, sum_w_min;
    int32_t K;          /* points per list; 0: the dense window */
    int32_t subsampled; /* 1: the sub-sampled path (needs the point lists) */
} vszip_bilateral_dither_cfg;
typedef struct vszip_bilateral_dither_plane {
    int32_t radius;
    float m, wmax, sum_w_min;
    const int16_t *points; /* device: 23 lists of K (x, y) pairs; NULL: dense */
    int32_t K;
} vszip_bilateral_dither_plane;

int vszip_bilateral_dither_derive(int is_float, int bits_per_sample, int radius, float thr, float flat, float wmin, float subspl,
                                  vszip_bilateral_dither_cfg *out, char *err, size_t err_cap);
int vszip_bilateral_dither_points(int radius, float subspl, int16_t *points, size_t capacity, int32_t *K);
int vszip_bilateral_dither(vszip_ctx *ctx, int dtype, int bits_per_sample, const vszip_plane *planes,
                           const vszip_bilateral_dither_plane *per_plane, int nplanes);

/*
 * Compress — MPEG-2 intra or JPEG artifacts: replaces processPlane of src/filters/compress.zig:458-515 (with processBlock :432-446:
 * fdctIslow :132-200, quantMpeg2 / dequantMpeg2 :215-254, quantJpeg / dequantJpeg :257-278, idctRows :296-356, idctColsPut :359-422)
 * as Compress(codec).getFrame calls it per plane (src/vapoursynth/compress.zig:23-48), QuantTables.buildMpeg2 / buildJpeg
 * (compress.zig:80-103) and the create-time checks of compressCreate (compress.zig(vs):77-110).
 *
 * vszip_compress_tables (device-free). The wrapper's arguments -> the tables of one clip, in natural raster order:
 *   mpeg2 (codec 0)  qmul[p][i] = (2 << 21) / (2 qscale M[i]), deq[p][i] = 2 qscale M[i] with M the default intra matrix, both p alike;
 *                    dc_scale = 8 >> dc_prec, dc_q = 8 dc_scale;
 *   jpeg (codec 1)   q = clamp((base_p[i] scale + 50) / 100, 1, 255) with scale = 5000 / quality below 50, else 200 - 2 quality;
 *                    deq[p][i] = q, qmul[p][i] = (1 << 21) / (8 q); dc_q = 64 and dc_scale = 8 are not used.
 * VSZIP_ERR_ARG with the wrapper's wording in `err` (may be NULL), in its order, only the chosen codec's parameters being
 * checked: "Compress: codec must be 0 (mpeg2) or 1 (jpeg).", "Compress: qscale must be between 1 and 31.", "Compress: dc_prec
 * must be between 0 and 3.", "Compress: quality must be between 1 and 100."; also for a NULL `out`. The wrapper's defaults are
 * codec 0, qscale 8, dc_prec 0, quality 50. (The type is `struct vszip_compress_tables`: C keeps struct tags apart from functions.)
 *
 * vszip_compress. 8-bit planes only; any number of planes of any sizes (w, h >= 1) in one call, so the planes of many frames fit.
 * chroma[i] != 0 selects table index 1 for planes[i] (the wrapper passes plane != 0); NULL: all luma. `ref` is unused. Planes
 * the wrapper does not process (chroma = False) are the host's copy. Per block: samples (jpeg: minus 128) -> forward DCT, two
 * passes -> quantise (64-bit products; mpeg2: DC (dc + dc_q / 2) / dc_q, AC with the deadzone and the 3/8 bias; jpeg: round to
 * nearest) -> dequantise (mpeg2: the magnitude times deq >> 4 with the sign restored, DC times dc_scale; jpeg: level times deq) ->
 * inverse DCT, two passes, a row with nothing beyond its first coefficient taking the short cut 8 c0 -> (jpeg: plus 128) -> clamp
 * to 0..255. Every pass stores 16-bit two's complement, all 32-bit arithmetic wraps: bit-exact with the reference. One fused pass,
 * a block per lane, no scratch. `tables` is HOST memory and is consumed before the call returns (it travels in the kernel
 * argument), so the caller may reuse it at once. Tables need not come from vszip_compress_tables, but must lie in the range it can
 * produce: 0 <= qmul <= 2^20 and 0 <= deq <= 32767 (with qmul >= 0 the quantiser works on the magnitude and restores the sign).
 * VSZIP_ERR_ARG: a NULL tables, src or dst, tables->codec outside 0..1, a multiplier outside those ranges, dc_q <= 0 with mpeg2, w
 * or h below 1, a pitch below w.
 * Asynchronous on the context stream. "Plane memory": reads stay inside [0, w) x h of src; only [0, w) x h of dst is written;
 * dst == src is allowed.
 */
struct vszip_compress_tables {
    int32_t codec;          /* 0 mpeg2, 1 jpeg */
    int32_t qmul[2][64];    /* reciprocal multipliers, natural raster order; [0] luma, [1] chroma (mpeg2: both alike) */
    int32_t deq[2][64];     /* dequantiser multipliers */
    int32_t dc_q, dc_scale; /* mpeg2 DC: encode divisor, decode multiplier (64 / 8 >> dc_prec); unused for jpeg */
};
int vszip_compress_tables(int codec, int qscale, int dc_prec, int quality, struct vszip_compress_tables *out, char *err, size_t err_cap);
int vszip_compress(vszip_ctx *ctx, const vszip_plane *planes, int nplanes, const struct vszip_compress_tables *tables, const uint8_t *chroma);

/*
 * PackRGB — planar RGB to one packed 32-bit plane for a previewer: replaces the two loops of Pack(is_rgb24).getFrame
 * (src/vapoursynth/packrgb.zig:33-63) and the format check of packrgbCreate (:88-97). One vszip_pack_rgb_frame per frame: r, g, b are
 * uint8_t planes (bits 8, RGB24) or uint16_t planes (bits 10, RGB30) of w x h samples with a pitch each, dst is the packed plane of
 * w x h uint32_t; all strides in elements of the plane's own sample type (dst_stride in 32-bit elements). Any number of frames of any
 * mix of sizes in one call. bits 8: dst = b | g << 8 | r << 16 | 255 << 24, in memory the bytes B, G, R, 0xFF. bits 10:
 * dst = b | g << 10 | r << 20 | 3 << 30 in uint32_t arithmetic, exactly as :60 writes it: nothing is masked, so a 16-bit sample above
 * 1023 runs into the neighbouring field and what is shifted beyond bit 31 is lost, as in the reference; that is not an error.
 * One streaming pass, no scratch. Asynchronous on the context stream. VSZIP_ERR_ARG: bits other than 8 or 10 ("PackRGB: only RGB24 and
 * RGB30 inputs are supported!", the reference's text), and, naming the frame ("PackRGB: frame 1: r, g, b and dst must not be NULL"), a
 * NULL plane, w or h below 1, a pitch below w. "Plane memory": reads stay inside [0, w) x h of r, g and b; only [0, w) x h of dst is
 * written; r, g and b may alias each other; dst may overlap no input.
 */
typedef struct vszip_pack_rgb_frame {
    const void *r, *g, *b; /* uint8_t (bits 8) or uint16_t (bits 10) planes, w x h each */
    ptrdiff_t r_stride, g_stride, b_stride;
    uint32_t *dst; /* w x h packed samples */
    ptrdiff_t dst_stride;
    int32_t w, h;
} vszip_pack_rgb_frame;
int vszip_pack_rgb(vszip_ctx *ctx, int bits, const vszip_pack_rgb_frame *frames, int nframes);

/*
 * ColorMap — Gray8 to false-colour RGB24 through a 256-entry table per channel: replaces the loop of colorMapGetFrame
 * (src/vapoursynth/color_map.zig:36-46) and the table build of colorMapCreate (:92-103). The palettes (the reference's 22 tables of
 * src/filters/color_map.zig) and the `color` range check 0..21 stay with the host that binds this library; the
 * frame properties of :48-52 are the host's, too.
 *
 * vszip_color_map_lut (host only, device-free). A palette of `len` points a channel (f32, nominally 0..1) -> lut[c][i], i = 0..255:
 * p = ((float)i * (float)(len - 1)) / 255.0f (a multiply, then a divide, both rounded to f32), lo = floor(p), hi = min(lo + 1, len - 1),
 * frac = p - lo, v = c[lo] + (c[hi] - c[lo]) * frac (the multiply and the add each rounded, never fused),
 * lut = trunc(fmaf(v, 255.0f, 0.5f)) (one fused operation). VSZIP_ERR_ARG, with the channel and the index in `err` (may be NULL):
 * len below 1 (or above 2^24), a NULL argument, and a table entry that is NaN or lands outside 0..255 (the reference's @trunc to u8
 * is undefined there), e.g. "ColorMap: g: table entry 255 (palette points 3 and 3) gives 258.05, outside 0..255".
 *
 * vszip_color_map. One vszip_color_map_frame per frame: src is a uint8_t plane of w x h, r, g, b the three output planes, a pitch
 * each; any number of frames of any mix of sizes in one call. Per sample s: r = lut[0][s], g = lut[1][s], b = lut[2][s]. `lut` is HOST
 * memory and is consumed before the call returns (it travels in the kernel argument), so the caller may overwrite it at once; it need
 * not come from vszip_color_map_lut. One streaming pass with the table in LDS, no scratch. Asynchronous on the context stream.
 * VSZIP_ERR_ARG: a NULL lut, and, naming the frame ("ColorMap: frame 1: src, r, g and b must not be NULL"), a NULL plane, w or h
 * below 1, a pitch below w. "Plane memory": reads stay inside [0, w) x h of src; only [0, w) x h of r, g and b is written; the three
 * outputs overlap neither each other nor src.
 */
typedef struct vszip_color_map_frame {
    const uint8_t *src;
    ptrdiff_t src_stride;
    uint8_t *r, *g, *b;
    ptrdiff_t r_stride, g_stride, b_stride;
    int32_t w, h;
} vszip_color_map_frame;
int vszip_color_map_lut(const float *r, const float *g, const float *b, int len, uint8_t lut[3][256], char *err, size_t err_cap);
int vszip_color_map(vszip_ctx *ctx, const vszip_color_map_frame *frames, int nframes, const uint8_t lut[3][256]);

/*
 * ImageUnpack — a decoder's packed, interleaved pixels to planes plus an alpha plane: replaces copyPixels and copyPixelsIndexed
 * (src/vapoursynth/image_read.zig:38-91) behind the switch of Read(alpha).getFrame (:285-345); the mirror of PackRGB. Reading, URL fetch,
 * decoding, the PNG colour chunks and every frame property stay with the host. One vszip_image_unpack_frame per
 * frame: src holds h rows of w pixels, a pixel's channels interleaved in the order the layout's name spells in memory; p[] and a are
 * the output planes of `dtype` samples. Planes are filled by NAME, as copyPixels reads .r / .g / .b: p[0] receives R (for BGR / BGRA
 * the pixel's third sample), p[1] G, p[2] B, a the alpha; the grey layouts write p[0] only and ignore p[1], p[2]. a == NULL drops the
 * channel; a is ignored by the layouts without alpha (GRAY, RGB, BGR). Any number of frames of any mix of sizes in one call, one
 * layout and type per call.
 *
 * src_stride is the one stride of this ABI given in BYTES (a 3-byte pixel does not divide a row pitch, and BMP rows are padded to 4
 * bytes); it is at least w x pixel bytes, which is what a dense zigimg image has. p_stride[] and a_stride are in samples of `dtype`.
 * src needs no alignment at all.
 *
 * Served (layout, dtype, src_bits), the arms of the reference's switch and no others; everything else is VSZIP_ERR_ARG:
 *   GRAY        VSZIP_U8  1 | 2 | 4 | 8   grayscale1 / 2 / 4 / 8          GRAY_ALPHA  VSZIP_U8 8 | VSZIP_U16 16   grayscale8Alpha / 16Alpha
 *   GRAY        VSZIP_U16 16              grayscale16                     RGB, RGBA   VSZIP_U8 8 | VSZIP_U16 16   rgb24 / rgba32 / rgb48 / rgba64
 *   BGR, BGRA   VSZIP_U8  8               bgr24 / bgra32                  RGBA        VSZIP_F32 32                float32 (four f32 a pixel)
 *   INDEXED     VSZIP_U8  8               indexed1 / 2 / 4 / 8: one index BYTE a pixel (zigimg's storage), palette = 256 x (R, G, B, A)
 * (BGR / BGRA with 16-bit samples, RGB / BGR / BGRA / the grey layouts with float samples: refused, the reference has no such format.)
 * Grey below 8 bits (scaleSample, :33-36): one sample a byte, the value in the low src_bits bits, higher bits ignored, output
 * v x 255 / (2^bits - 1), that is x 255, x 85, x 17. Everywhere else src_bits equals the sample width and samples pass through bit
 * for bit; float samples pass as bits, NaN payloads kept. `palette` is HOST memory, always 256 entries (no index can leave it; the host
 * fills the entries its image does not define) and is consumed before the call returns (it travels in the kernel argument); it is NULL
 * for every other layout. indexed16 is not served (the reference writes the palette's 8-bit channels into 16-bit planes; DESIGN.md
 * 3.17): an index width other than 8 is VSZIP_ERR_ARG with a text that says so.
 *
 * One streaming pass, no scratch. Asynchronous on the context stream. VSZIP_ERR_ARG: a combination that is not served, a palette
 * where none belongs or none where one does, and, naming the frame ("ImageUnpack: frame 1: src, p[0], p[1] and p[2] must not be
 * NULL"), a NULL required plane, w or h below 1, a plane pitch below w, a source pitch below the row's bytes. "Plane memory": reads stay
 * inside the w x pixel-bytes of each of the h source rows (source pitch padding is never read); only [0, w) x h of each output plane
 * is written; the outputs overlap neither each other nor src. Every base and pitch is served: a fast path for frames whose output
 * bases and pitches (in bytes) are multiples of 16, and a slower one with the same bits.
 */
enum { VSZIP_IMG_GRAY = 0, VSZIP_IMG_GRAY_ALPHA = 1, VSZIP_IMG_RGB = 2, VSZIP_IMG_RGBA = 3, VSZIP_IMG_BGR = 4, VSZIP_IMG_BGRA = 5, VSZIP_IMG_INDEXED = 6 };
typedef struct vszip_image_unpack_frame {
    const void *src;      /* w x h packed pixels, channels interleaved in the layout's memory order */
    ptrdiff_t src_stride; /* in BYTES */
    void *p[3];           /* p[0]: grey or R; p[1], p[2]: G, B (ignored for the grey layouts) */
    void *a;              /* alpha plane, or NULL: the channel is dropped */
    ptrdiff_t p_stride[3], a_stride; /* in samples of the output type */
    int32_t w, h;
} vszip_image_unpack_frame;
int vszip_image_unpack(vszip_ctx *ctx, int layout, int dtype, int src_bits, const vszip_image_unpack_frame *frames, int nframes, const uint8_t palette[256][4]);

/*
 * PlaneMinMax — replaces filter.minMax / minMaxRef / minMaxNoThr / minMaxNoThrRef
 * (src/filters/planeminmax.zig:72-133) called from src/vapoursynth/planeminmax.zig:60-77.
 * minthr == maxthr == 0 is the exact path; otherwise the histogram-percentile rule of
 * minMaxImpl (:43-57). vmin/vmax hold integers for integer clips and idx/65535 (as f32)
 * for float clips, exactly the values the wrapper stores in psmMin/psmMax (:59-68).
 */
int vszip_plane_minmax(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes,
                       float minthr, float maxthr, int bits_per_sample,
                       double *vmin, double *vmax, double *diff);
/* ... and without the synchronise: pinned_results[i][0] = min, [i][1] = max, [i][2] = diff (see vszip_plane_average_async); [i][3] is scratch
 * (a thresholded sweep may leave a marker there) */
int vszip_plane_minmax_async(vszip_ctx *ctx, int dtype, const vszip_plane *planes, int nplanes,
                             float minthr, float maxthr, int bits_per_sample, double *pinned_results);

/*
 * Bilateral — replaces filter.bilateral (src/filters/bilateral.zig:81) and the create-time
 * work of bilateralCreate (src/vapoursynth/bilateral.zig:104-231).
 *
 * One vszip_bilateral_cfg per PLANE INDEX of the clip (Y,U,V / R,G,B):
 *   vszip_bilateral_derive  fills sigmaS/sigmaR/process/algorithm/pbficnum/radius/step/samples
 *                           from the user arrays (already expanded to 3 entries with hz.getArray's
 *                           repeat-last rule; sigmaS is passed raw with its element count because
 *                           its chroma default depends on the subsampling, :104-124). Host only.
 *                           Returns VSZIP_ERR_ARG for the cases bilateralCreate rejects.
 *   vszip_bilateral_luts    builds gs_lut ((radius+1)^2) and gr_lut (hist_len) exactly as
 *                           bilateral.zig:306-339 and uploads them (device memory owned by the
 *                           caller: vszip_dev_free). hist_len = 1 << bits, 65536 for float clips.
 *   vszip_bilateral         filters `nplanes` planes; cfgs[i] is the config of planes[i]'s plane
 *                           index. planes[i].ref == NULL means ref == src (no joint clip).
 *                           peak = hist_len - 1 as float (:101-102).
 * Planes with process == 0 (sigmaS == 0 or sigmaR == 0) are pass-through in the reference
 * (newVideoFrame2 copies them); copy them with vszip_copy_d2d_2d.
 */
typedef struct vszip_bilateral_cfg {
    double sigmaS;
    double sigmaR;
    int32_t process;
    int32_t algorithm; /* 1 = PBFIC, 2 = truncated window */
    int32_t pbficnum;
    int32_t radius;
    int32_t step;
    int32_t samples;
    float *gs_lut; /* device */
    float *gr_lut; /* device */
} vszip_bilateral_cfg;

int vszip_bilateral_derive(const double *sigmaS, int n_sigmaS, const double *sigmaR3, const int *algorithm3,
                           const int *pbficnum3, int is_yuv, int subsampling_w, int subsampling_h,
                           const int *planes3, vszip_bilateral_cfg *out3);
int vszip_bilateral_luts(vszip_ctx *ctx, vszip_bilateral_cfg *cfg, int hist_len);
int vszip_bilateral(vszip_ctx *ctx, int dtype, const vszip_plane *planes,
                    const vszip_bilateral_cfg *const *cfgs, int nplanes, float peak);

/*
 * Chained pixel filters on resident planes (frames stay on the device between
 * chained vszip filters). Every filter entry point takes device pointers, so a host may simply call them one
 * after another on one context; vszip_chain_run does that for the frame-in / frame-out filters in ONE call and
 * owns the intermediate planes: upload once (vszip_copy_h2d_2d), vszip_chain_run, download once. What the
 * reference does as separate filter instances with a host frame in between — clip.vszip.Bilateral().vszip.BoxBlur()
 * = bilateralGetFrame (src/vapoursynth/bilateral.zig) feeding BoxBlur's getFrame (src/vapoursynth/boxblur.zig:29-50).
 *   stages[s].process[k]  whether stage s filters plane slot k (0..2: Y/U/V or R/G/B); other planes pass through,
 *                         as the reference's newVideoFrame2 plane copy does;
 *   planes[i]             src = resident input, dst = where the chain's result goes; plane_slot[i] in 0..2 picks
 *                         the per-plane parameters (a table may hold the planes of many frames).
 * libvszip.so applies the same scheme across filter INSTANCES: a vszip filter created on the output of another
 * vszip pixel filter runs that filter's kernels itself on its own upload ("Fused chains").
 */
enum { VSZIP_STAGE_BOXBLUR = 0, VSZIP_STAGE_BILATERAL = 1, VSZIP_STAGE_LIMITER = 2 };
typedef struct vszip_chain_stage {
    int32_t kind;
    int32_t process[3];
    int32_t hradius, hpasses, vradius, vpasses; /* BoxBlur */
    const struct vszip_bilateral_cfg *bilateral[3]; /* Bilateral: per plane slot, LUTs resident (vszip_bilateral_luts) */
    float peak;                                     /* Bilateral: as vszip_bilateral */
    double lo[3], hi[3];                            /* Limiter: resolved bounds per plane slot */
} vszip_chain_stage;
int vszip_chain_run(vszip_ctx *ctx, int dtype, const vszip_chain_stage *stages, int nstages,
                    const vszip_plane *planes, const int *plane_slot, int nplanes);

/*
 * vszip_chain_ops: resident chains over EVERY frame-in / frame-out filter of this header. What vszip_chain_run is for BoxBlur, Bilateral and
 * Limiter, for the filters added since as well: Checkmate -> MosquitoNR -> Deband, Compress -> MosquitoNR, CLAHE -> Limiter, BoxBlur -> CombMask in
 * one call, with the library owning every intermediate plane. vszip_chain_run is a translation of its stages into ops followed by this call: its
 * stage struct is flat and per plane SLOT, while Deband's grain pointer, MosquitoNR's strengths and Compress's chroma flags are per table ENTRY and
 * Checkmate and CombMask read neighbouring FRAMES, so the newer kinds live here.
 *
 * An op is (kind, process[3], params): process[k] as in vszip_chain_stage, and params points to ONE small struct of the kind, which holds exactly
 * the arguments of that kind's entry point (the structs below, named after the VSZIP_STAGE_ number they belong to). All pointers are read before the
 * call returns and may be reused at once, as with the entry points themselves. dtype is one sample type for the whole chain; bits_per_sample is what
 * vszip_mosquito_nr and vszip_bilateral_dither take (8 for VSZIP_U8, 9..16 for VSZIP_U16, ignored for VSZIP_F32) and is not looked at when neither
 * kind occurs.
 *
 * Not chain ops: the two-input joins (vszip_limit_filter, vszip_adaptive_binarize, vszip_bilateral and vszip_bilateral_dither with a `ref` clip) and
 * the filters whose output has another format than their input (vszip_pack_rgb, vszip_color_map, vszip_image_unpack); a chain is one clip in, the
 * same format out. The metric filters return scalars. A host runs those on the chain's dst planes, which are resident too.
 *
 * Rules.
 * 1. Per-plane parameter arrays run beside the plane table. MosquitoNR's strength / restore / radius / chroma, Deband's per, BilateralDither's per
 *    and Compress's chroma have nplanes entries each, entry i belonging to planes[i], exactly as the underlying entry points index them. The chain
 *    compacts them to the entries the op processes; entries of slots the op skips are not read. A NULL where the entry point allows NULL
 *    (MosquitoNR's and Compress's chroma) keeps its meaning. Bilateral's cfg and Limiter's lo / hi stay per plane slot, as in vszip_chain_stage.
 * 2. Plane semantics are vszip_chain_run's. An op filters the entries whose slot it processes and passes the others through; the last op that writes
 *    an entry writes the caller's dst; an entry no op writes is copied when dst != src. Every op reads and writes different memory: an entry
 *    with two or more writers ping-pongs between the two halves of a region of its own in the context's chain buffer (dense rows at a 256-byte
 *    pitch, grow-only), so the "dst must not overlap src" rules of Deband, MosquitoNR and the stencil filters hold by construction. What stays with
 *    the caller: a dst plane overlaps no src plane of the table (dst == src of the same entry is fine where every op that writes dst allows it on
 *    its own: a chain of one Limiter, say). planes[i].ref is not used: BilateralDither runs without `ref`, Bilateral with ref == src, and CombMask's
 *    previous frame comes from the table (rule 3).
 * 3. The table is a clip. frame[i] is the frame number of entry i; `frame` may be NULL when no op is temporal. The temporal ops are Checkmate, and
 *    CombMask with mthresh > 0. With one present: within every plane slot the frame numbers form one contiguous range fmin..fmax, each
 *    (slot, frame) pair occurs once, and all entries of a slot have the same w x h; anything else is VSZIP_ERR_ARG. A temporal op finds the
 *    neighbours of entry i among the entries of the same slot and takes them where the PREVIOUS WRITING OP LEFT THEM (the caller's src if none
 *    wrote yet): BoxBlur -> Checkmate is Checkmate on the blurred clip. Frame indices are clamped to the table's range exactly as the wrappers
 *    clamp to the clip: Checkmate max(fmin, n - k) and min(n + k, fmax); CombMask max(fmin, n - 1), so frame fmin is its own `ref` and its motion
 *    mask is all zero. A host passes whole clips or, for a window of one, the frames around it. No op reads what it writes: all entries of a slot
 *    have been written equally often, an op reads only the halves earlier ops wrote (or src) and writes the other halves or the callers' dst
 *    (csrc/chain_plan.hpp derives it; tests/chain_plan_check.cpp sweeps it).
 * 4. Nothing is queued before the chain is known to be well formed. Checked for every op before the first launch, VSZIP_ERR_ARG with a
 *    vszip_last_error text that names the op index ("chain: op 2 (Compress) does not take sample type 1"): the kind number; NULL params, and a NULL
 *    pointer inside params where the entry point takes none (MosquitoNR's strength / restore / radius, Deband's and BilateralDither's per,
 *    Compress's tables, Bilateral's cfg of a slot the op processes); the dtype a kind accepts (U8 only for CombMask, CombMaskMT, Checkmate and
 *    Compress, whose entry points take no dtype and would read wider planes as bytes; U8 / U16 for CLAHE; U16 / F32 for Deband; U8 / U16 / F32 for
 *    MosquitoNR and BilateralDither; U8 / U16 / F16 / F32 for BoxBlur and Bilateral; those and U32 for Limiter); bits_per_sample against dtype
 *    where a kind uses it; the frame-table conditions of rule 3; and per plane a NULL src or dst, w or h below 1, a slot outside 0..2
 *    ("chain: bad plane 3").
 * 5. Value checks stay with the entry points: thresholds out of range, planes too small for a filter, a radius too large. Their status and their
 *    wording come through unchanged. After such a failure the ops before the failing one have run and the contents of the dst planes are
 *    unspecified; the next call on the context is correct all the same.
 * Asynchronous on the context stream (growing the chain buffer drains it first).
 */
enum { VSZIP_STAGE_CLAHE = 3, VSZIP_STAGE_COMB_MASK = 4, VSZIP_STAGE_COMB_MASK_MT = 5, VSZIP_STAGE_CHECKMATE = 6, VSZIP_STAGE_MOSQUITO_NR = 7, VSZIP_STAGE_DEBAND = 8,
       VSZIP_STAGE_BILATERAL_DITHER = 9, VSZIP_STAGE_COMPRESS = 10 };
typedef struct vszip_chain_op {
    int32_t kind;       /* VSZIP_STAGE_* */
    int32_t process[3]; /* per plane slot */
    const void *params; /* the struct of `kind` below */
} vszip_chain_op;
typedef struct vszip_chain_boxblur { int32_t hradius, hpasses, vradius, vpasses; } vszip_chain_boxblur;
typedef struct vszip_chain_bilateral {
    const struct vszip_bilateral_cfg *cfg[3]; /* per plane slot, LUTs resident */
    float peak;
} vszip_chain_bilateral;
typedef struct vszip_chain_limiter { double lo[3], hi[3]; /* per plane slot */ } vszip_chain_limiter;
typedef struct vszip_chain_clahe { uint32_t limit; int32_t tiles_x, tiles_y; } vszip_chain_clahe;
typedef struct vszip_chain_comb_mask { int32_t cthresh, mthresh, expand, metric; } vszip_chain_comb_mask;
typedef struct vszip_chain_comb_mask_mt { int32_t thy1, thy2; } vszip_chain_comb_mask_mt;
typedef struct vszip_chain_checkmate { int32_t thr, tmax, tthr2; } vszip_chain_checkmate;
typedef struct vszip_chain_mosquito_nr {
    const int32_t *strength, *restore, *radius; /* nplanes entries each */
    const uint8_t *chroma;                      /* nplanes entries, or NULL */
} vszip_chain_mosquito_nr;
typedef struct vszip_chain_deband {
    const vszip_deband_plane *per; /* nplanes entries */
    int32_t sample_mode, blur_first;
    float angle_boost, max_angle;
    int32_t max_offset;
} vszip_chain_deband;
typedef struct vszip_chain_bilateral_dither { const vszip_bilateral_dither_plane *per; /* nplanes entries */ } vszip_chain_bilateral_dither;
typedef struct vszip_chain_compress {
    const struct vszip_compress_tables *tables;
    const uint8_t *chroma; /* nplanes entries, or NULL */
} vszip_chain_compress;
int vszip_chain_ops(vszip_ctx *ctx, int dtype, int bits_per_sample, const vszip_chain_op *ops, int nops,
                    const vszip_plane *planes, const int *plane_slot, const int *frame, int nplanes);

/*
 * SSIMULACRA2 — replaces filter_ssim.process (src/filters/ssimulacra2.zig:46) called from
 * ssimulacra2GetFrame (src/vapoursynth/ssimulacra2.zig:40-66). Inputs are linear-light
 * RGBS planes (what hz.toRGBS + sRGBtoLinearRGB hand to the kernel, :115-118): ref3 / dis3
 * are HOST arrays of 3 * npairs device pointers (R,G,B of pair 0, R,G,B of pair 1, ...),
 * all planes w x h with the same stride (elements). scores[npairs] receives the value the
 * wrapper stores in the "SSIMULACRA2" frame property. Synchronises the stream.
 */
int vszip_ssimulacra2(vszip_ctx *ctx, const float *const *ref3, const float *const *dis3,
                      ptrdiff_t stride, int w, int h, int npairs, double *scores);

/*
 * SSIMULACRA2 with its colour pre-stage on the device — additionally replaces, for the clips that
 * need no resampler, what ssimulacraCreate hangs in front of the kernel on the host:
 * hz.toRGBS (src/helper.zig:225-243: resize.Bicubic(format=RGBS, matrix_in=709|601)) and
 * sRGBtoLinearRGB (src/vapoursynth/ssimulacra2.zig:132-162: std.SetFrameProp(_Transfer=13) +
 * resize.Bicubic(transfer=LINEAR)), i.e. zimg's integer -> float conversion (full range for RGB,
 * limited for Gray), Gray -> R = G = B, and the sRGB EOTF through zimg's approximate-gamma table
 * (VapourSynth's resize default). The source planes are uploaded as they are (8/16-bit samples: a
 * quarter / half of the RGBS bytes), the conversion is fused into the first SSIMULACRA2 pass.
 *   family     VSZIP_CF_RGB (3 planes per frame), VSZIP_CF_GRAY (1 plane per frame) or — round 3 — VSZIP_CF_YUV
 *              (3 planes, chroma subsampled by 2^ssw x 2^ssh): zimg's integer -> float conversion per plane, the
 *              chroma planes brought to 4:4:4 with its Catmull-Rom resampler (resize.Bicubic: b = 0, c = 0.5;
 *              horizontal pass first, two interleaved FMA accumulators per sample — vszip_resample_table below),
 *              the YUV -> RGB matrix as an FMA chain, then the transfer table. Restated from zimg's published
 *              algorithm and pinned by the reference's seven YUV SSIMULACRA2 goldens (tests/test_oracle_zimg_goldens.py);
 *   dtype/bits VSZIP_U8 (8), VSZIP_U16 (9..16) or VSZIP_F32 (f16 is rejected by the wrapper, :106-113);
 *   limited    integer samples are limited range (zimg's default for Gray and YUV) or full (RGB);
 *   linearize  0 when frame 0 carries _Transfer == LINEAR (:139-141), else 1;
 *   YUV only:  ssw / ssh   log2 chroma subsampling (0..2). A sited chroma plane (chroma_loc != center) lies half a LUMA
 *                          sample off the centre of its 2^ss luma samples whatever ss — zimg's rule (0.5 / 2^ss chroma
 *                          samples); ss = 2 (4:1:0, 4:1:1) is not covered by any reference golden, and libvszip.so
 *                          leaves such clips to the host's resize;
 *              matrix      _Matrix of the clip's frames if set and specified, else what hz.toRGBS passes as matrix_in
 *                          (1 = BT.709 if height > 650 else 6 = BT.601; src/helper.zig:231) — VapourSynth's resize
 *                          lets a frame property win over the *_in argument; supported: 1, 5, 6, 9;
 *              chroma_loc  _ChromaLocation (0 left — the default —, 1 center, 2 top-left, 3 top, 4 bottom-left, 5 bottom);
 *              chroma_stride  row pitch of the U and V planes, elements.
 * ref_planes / dis_planes: HOST arrays of npairs * (3 | 1) device plane pointers, same stride (elements).
 */
enum { VSZIP_CF_RGB = 0, VSZIP_CF_GRAY = 1, VSZIP_CF_YUV = 2 };
typedef struct vszip_ssim_source {
    int family, dtype, bits, limited, linearize;
    int ssw, ssh, matrix, chroma_loc; /* VSZIP_CF_YUV */
    ptrdiff_t chroma_stride;          /* VSZIP_CF_YUV */
} vszip_ssim_source;
int vszip_ssimulacra2_src(vszip_ctx *ctx, const vszip_ssim_source *fmt, const void *const *ref_planes,
                          const void *const *dis_planes, ptrdiff_t stride, int w, int h, int npairs, double *scores);
/* The pre-stage alone: one frame's planes -> linear-light RGBS planes (dst3: R, G, B device pointers).
 * Asynchronous on the context stream. */
int vszip_to_rgbs_linear(vszip_ctx *ctx, const vszip_ssim_source *fmt, const void *const *src_planes, ptrdiff_t src_stride,
                         float *const *dst3, ptrdiff_t dst_stride, int w, int h);
/* zimg's Catmull-Rom table for one axis of an upscale (device-free): output sample i = sum_k coef4[4 i + k] *
 * src[min(left[i] + k, src_dim - 1)], accumulated as (c0 x0 + fma(c2, x2, .)) + (c1 x1 + fma(c3, x3, .)).
 * shift: position offset in source samples (4:2:0 left-sited chroma -> luma grid: 0.25 horizontally, 0 vertically). */
int vszip_resample_table(int src_dim, int dst_dim, double shift, int32_t *left, float *coef4);

/*
 * EEDI3 / EEDI3H — replaces processPlane (src/vapoursynth/eedi3.zig:26-140) with its kernels
 * interpLine / vcheckLine (src/filters/eedi3.zig:349-592, 915-1046) and, for horizontal != 0,
 * the transposes of :220-246. 32-bit float planes only (createImpl :316-319).
 * planes[i].src is src_w x src_h; planes[i].dst is src_w x (dh ? 2*src_h : src_h) for EEDI3 and
 * (dh ? 2*src_w : src_w) x src_h for EEDI3H. `field` is the frame's resolved parity 0/1
 * (getFrame :166-172 folds _FieldBased and field 2/3 into it). With dh = 0 the source rows (EEDI3H:
 * columns) of parity `field` are replaced by the interpolation; the vertical form does not read them at all
 * ("Plane memory", clause 2), so a host need not upload them. sclips[i] (may be NULL, as may
 * the array) has dst's geometry. Parameters are the user-level ones (defaults: alpha .2,
 * beta .25, gamma 20, nrad 2, mdis 20, hp 0, vcheck 2, vthresh 32/64/4); the scaling of
 * :465-473 happens inside. Errors mirror createImpl's messages.
 */
typedef struct vszip_eedi3_params {
    int32_t dh;
    float alpha, beta, gamma;
    int32_t nrad, mdis, hp, vcheck;
    float vthresh0, vthresh1, vthresh2;
} vszip_eedi3_params;

int vszip_eedi3(vszip_ctx *ctx, const vszip_plane *planes, const float *const *sclips,
                const ptrdiff_t *sclip_strides, int nplanes, int field, int horizontal,
                const vszip_eedi3_params *params);
/* The same with the `mclip` mask (createImpl :393-433, buildBmask src/filters/eedi3.zig:285-304):
 * mclips[i] (may be NULL, as may the array) is an 8-bit plane with the geometry of planes[i].src —
 * the wrapper passes the same Gray mask for every plane, like getFrame :215-218 — strides in
 * bytes == elements. Pixels whose +-mdis neighbourhood holds no mask sample keep the plain
 * vertical cubic. */
int vszip_eedi3_mclip(vszip_ctx *ctx, const vszip_plane *planes, const float *const *sclips,
                      const ptrdiff_t *sclip_strides, const uint8_t *const *mclips,
                      const ptrdiff_t *mclip_strides, int nplanes, int field, int horizontal,
                      const vszip_eedi3_params *params);

/*
 * XPSNR — replaces filter.getWSSE (src/filters/xpsnr.zig:376) called from XPSNR(T).getFrame
 * (src/vapoursynth/xpsnr.zig:72-82): org3/rec3 are host arrays of num_comps device plane
 * pointers (u8 or u16 samples: bytes_per_sample 1 or 2, depth 8 or 10), prev1/prev2 the luma of
 * reference frames n-1 / n-2 or NULL (n == 0/1, or temporal off). wsse3 receives wsse64[0..2].
 * Synchronises the stream. vszip_xpsnr_value / _average are getFrameXPSNR / getAvgXPSNR
 * (:359-374), host-only helpers for the wrapper's props and its per-clip summary.
 */
int vszip_xpsnr_wsse(vszip_ctx *ctx, int bytes_per_sample, const void *const *org3, const void *const *rec3,
                     const void *prev1, const void *prev2, const int *width3, const int *height3,
                     const ptrdiff_t *stride3, int depth, int num_comps, unsigned frame_rate, int temporal,
                     uint64_t *wsse3);
/* The same for a batch of frames in one launch (what a host that already holds several frames of
 * the clip calls; frame f of the batch is exactly vszip_xpsnr_wsse on its own pointers):
 * org3/rec3 hold nframes*num_comps plane pointers, frame-major; prev1/prev2 (arrays of nframes
 * luma pointers, entries or the arrays themselves may be NULL) are per frame; every frame shares
 * the geometry. wsse3 receives 3 values per frame. */
int vszip_xpsnr_wsse_batch(vszip_ctx *ctx, int bytes_per_sample, int nframes, const void *const *org3,
                           const void *const *rec3, const void *const *prev1, const void *const *prev2,
                           const int *width3, const int *height3, const ptrdiff_t *stride3, int depth,
                           int num_comps, unsigned frame_rate, int temporal, uint64_t *wsse3);
double vszip_xpsnr_value(uint64_t wsse, uint64_t width, uint64_t height, int depth);
double vszip_xpsnr_average(double sum_wdist, double sum_xpsnr, uint64_t width, uint64_t height, int depth,
                           uint64_t num_frames);

#ifdef __cplusplus
}
#endif
#endif /* VSZIP_HIP_H */
