// Every switch of libvszip_hip.so, ONE line each: VSZIP_OPT(field, "ENVIRONMENT NAME", default).
// They are read from the environment ONCE, in vszip_ctx_create (ctx.hip: the only getenv in csrc/), into
// ctx->opt; vszip_ctx_set_option changes one on a live context (the path-agreement tests do). No dispatch
// parses strings per call and none races a host's setenv (VERDICT r3 item 6, ADVICE r3).
//
// VSZIP_OPT      shipped: user-facing knobs and the selectors between the kernels a default build contains
//                (each selectable path is a real fallback for some geometry / sample type; the tests force it
//                on geometries the default would not route there and compare the results)
// VSZIP_DEV_OPT  only in a -DVSZIP_DEV_VARIANTS build (tools/ab*.sh pass it): measured-slower kernels and sweep
//                knobs. In the default build the field is a compile-time constant and the kernels are not compiled.
//
// Flags: unset / "0" / "" = off, anything else = on. Integers: atoi.

// ---- user-facing (INTEGRATION.md "Environment") ----
VSZIP_OPT(staging, "VSZIP_STAGING", 0)                    // 1 | "pinned": host copies go through the context's pinned arena
VSZIP_OPT(placement, "VSZIP_PLACEMENT", 1)                // large vszip_dev_alloc requests: the fastest of a few probed candidate allocations (ctx.hip)
VSZIP_OPT(placement_min_mib, "VSZIP_PLACEMENT_MIN_MIB", 256)    // ... from this size on
VSZIP_OPT(placement_tries, "VSZIP_PLACEMENT_TRIES", 24)         // ... looking at no more candidates than this (and never holding more than a quarter of the free device memory)
VSZIP_OPT(placement_budget_ms, "VSZIP_PLACEMENT_BUDGET_MS", 300)  // ... and never starting another candidate after this many milliseconds of search
VSZIP_OPT(clahe_scratch_mib, "VSZIP_CLAHE_SCRATCH_MIB", 1024)  // CLAHE: histogram + LUT storage of one plane group at most (a larger table runs in several groups; a plane is never split)
VSZIP_OPT(deband_scratch_mib, "VSZIP_DEBAND_SCRATCH_MIB", 1024)  // Deband sample mode 7: gradient-angle planes of one plane group at most (a larger table runs in several groups; a plane is never split)
VSZIP_OPT(deband_lowbit_scratch_mib, "VSZIP_DEBAND_LOWBIT_SCRATCH_MIB", 1024)  // Deband under 16 bits: the two 16-bit intermediates of one plane group at most (a larger table runs in several groups; a plane is never split)

// ---- path selectors between shipped kernels ----
VSZIP_OPT(scan_mode, "VSZIP_SCAN_MODE", 0)                // BoxBlur CT: 0 ring kernel, 1 generic kernel + shuffle scan, 2 generic kernel + DPP scan
VSZIP_OPT(ct_u8_px8, "VSZIP_CT_U8_PX8", 0)               // BoxBlur CT on 8-bit planes: 8 pixels a lane at every width (16 when every width is whole 16-pixel groups otherwise)
VSZIP_OPT(boxblur_no_ct_h, "VSZIP_BOXBLUR_NO_CT_H", 0)    // a horizontal-only integer blur of r <= 22 through the RT row kernel instead of the ring kernel with a one-row window (round 4)
VSZIP_OPT(rt_no_hsmall, "VSZIP_RT_NO_HSMALL", 0)
VSZIP_OPT(rt_no_ichain, "VSZIP_RT_NO_ICHAIN", 0)
VSZIP_OPT(rt_no_fchain, "VSZIP_RT_NO_FCHAIN", 0)
VSZIP_OPT(rt_ichain_all, "VSZIP_RT_ICHAIN_ALL", 0)
VSZIP_OPT(rt_fchain_all, "VSZIP_RT_FCHAIN_ALL", 0)
VSZIP_OPT(rt_no_banded, "VSZIP_RT_NO_BANDED", 0)          // integer pass chains: no row bands (one wave per column group walks the whole plane)
VSZIP_OPT(bilateral_no_lds16, "VSZIP_BILATERAL_NO_LDS16", 0)
VSZIP_OPT(bilateral_no_walk, "VSZIP_BILATERAL_NO_WALK", 0)
VSZIP_OPT(bilateral_no_fine, "VSZIP_BILATERAL_NO_FINE", 0)
VSZIP_OPT(eedi3_force_overlap, "VSZIP_EEDI3_FORCE_OVERLAP", 0)
VSZIP_OPT(eedi3_no_overlap, "VSZIP_EEDI3_NO_OVERLAP", 0)
VSZIP_OPT(minmax_no_predict, "VSZIP_MINMAX_NO_PREDICT", 0)   // thresholded PlaneMinMax on 16-bit / float planes: always the two sweeps (no single-read sweep over the ranges the previous call of the same shape predicts)
VSZIP_OPT(ssim_no_yuv420_lds, "VSZIP_SSIM_NO_YUV420_LDS", 0)  // SSIMULACRA2 on 4:2:0 / 4:2:2 / 4:4:4 integer clips: the fused tile kernel (what the other YUV formats take) instead of the persistent pre-stage passes with the transfer table in LDS + the f32 pyramid pass (rounds 5, 6)
VSZIP_OPT(deband_path, "VSZIP_DEBAND_PATH", 0)            // Deband gathers: 0 by the call's max_offset (LDS tile up to 32, else global memory), 1 the LDS tile wherever its halo covers max_offset, 2 always global memory
VSZIP_OPT(bilateral_dither_path, "VSZIP_BILATERAL_DITHER_PATH", 0)  // BilateralDither taps: 0 the LDS tile where tile + halo (+ ref tile) fit its LDS budget, else global memory; 1 the LDS tile wherever it fits; 2 always global memory
VSZIP_OPT(depth_waves, "VSZIP_DEPTH_WAVES", 0)            // Depth error diffusion: 0 the workgroup by the plane's rows (4 waves up to 256 rows, else 16), 4 | 16 that workgroup for every plane

// ---- development variants (measured losers and sweep knobs) ----
// (round 5: selectors whose alternative is never the faster one on any geometry of tools/cliff_sweep.py; the kernels that geometry rules still route to stay in the default build, only the switch that FORCES them is a development variant)
VSZIP_DEV_OPT(boxblur_no_float_ring, "VSZIP_BOXBLUR_NO_FLOAT_RING", 0)
VSZIP_DEV_OPT(boxblur_float_bottom_strip, "VSZIP_BOXBLUR_FLOAT_BOTTOM_STRIP", 0)
VSZIP_DEV_OPT(rt_hrow, "VSZIP_RT_HROW", 0)
VSZIP_DEV_OPT(rt_no_virt, "VSZIP_RT_NO_VIRT", 0)
VSZIP_DEV_OPT(rt_no_vring, "VSZIP_RT_NO_VRING", 0)
VSZIP_DEV_OPT(rt_ichain_bands, "VSZIP_RT_ICHAIN_BANDS", 0)    // integer pass chains: this many row bands per plane (0: chosen by the library)
VSZIP_DEV_OPT(bilateral_no_cubic, "VSZIP_BILATERAL_NO_CUBIC", 0)
VSZIP_DEV_OPT(bilateral_untiled, "VSZIP_BILATERAL_UNTILED", 0)
VSZIP_DEV_OPT(bilateral_no_walk36, "VSZIP_BILATERAL_NO_WALK36", 0)
VSZIP_DEV_OPT(vcheck_global, "VSZIP_VCHECK_GLOBAL", 0)
VSZIP_DEV_OPT(eedi3_no_fixed, "VSZIP_EEDI3_NO_FIXED", 0)
VSZIP_DEV_OPT(ssim_one_stream, "VSZIP_SSIM_ONE_STREAM", 0)
VSZIP_DEV_OPT(xpsnr_blocks, "VSZIP_XPSNR_BLOCKS", 0)
VSZIP_DEV_OPT(xpsnr_unpacked, "VSZIP_XPSNR_UNPACKED", 0)
VSZIP_DEV_OPT(xpsnr_host_weigh, "VSZIP_XPSNR_HOST_WEIGH", 0)
VSZIP_DEV_OPT(rt_fused, "VSZIP_RT_FUSED", 0)              // boxblur_rt_hmulti_kernel: all passes of an axis with the row in registers — slower than a launch per pass
VSZIP_DEV_OPT(rt_vsmall, "VSZIP_RT_VSMALL", 0)            // boxblur_rt_vsmall_kernel: overtaken by the per-pass LDS ring
VSZIP_DEV_OPT(rt_vsmall_max, "VSZIP_RT_VSMALL_MAX", 2)
VSZIP_DEV_OPT(rt_no_vsmall, "VSZIP_RT_NO_VSMALL", 0)
VSZIP_DEV_OPT(rt_vband, "VSZIP_RT_VBAND", 0)              // sweep knob: band height of boxblur_rt_vband_kernel
VSZIP_DEV_OPT(rt_vring_maxr, "VSZIP_RT_VRING_MAXR", 0)    // sweep knob: largest radius that takes the vertical LDS ring
VSZIP_DEV_OPT(rt_group_mb, "VSZIP_RT_GROUP_MB", 0)        // Infinity-Cache sized plane groups: no gain measured
VSZIP_DEV_OPT(ring_periods, "VSZIP_RING_PERIODS", 0)      // sweep knob: ring periods per band of boxblur_ct_ring_kernel
VSZIP_DEV_OPT(minmax_single_read, "VSZIP_MINMAX_SINGLE_READ", 0)  // hist_sample_kernel: slower on two of three contents
