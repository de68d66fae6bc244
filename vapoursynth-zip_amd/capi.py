"""ctypes binding of include/vszip_hip.h (libvszip_hip.so) + small numpy helpers.

This is plumbing for tests, bench.py and the Python host mirror; the product is
the shared library. Loading fails loudly when the HIP library is missing — there
is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / "libvszip_hip.so"

U8, U16, F16, F32 = 0, 1, 2, 3
OK, ERR_ARG, ERR_HIP, ERR_UNSUPPORTED, ERR_NOMEM = 0, -1, -2, -3, -4
_NP2DT = {np.dtype(np.uint8): U8, np.dtype(np.uint16): U16, np.dtype(np.float16): F16, np.dtype(np.float32): F32, np.dtype(np.uint32): 4}
_DT2NP = {v: k for k, v in _NP2DT.items()}


VARIANTS_ABSENT: dict = {}  # development-variant switches a test asked for that this build does not contain -> how often (Device.variant)


class VszipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


class Plane(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("dst", C.c_void_p), ("ref", C.c_void_p),
        ("src_stride", C.c_ssize_t), ("dst_stride", C.c_ssize_t), ("ref_stride", C.c_ssize_t),
        ("w", C.c_int32), ("h", C.c_int32),
    ]


class TemporalNbrs(C.Structure):
    """vszip_temporal_nbrs"""
    _fields_ = [
        ("p2", C.c_void_p), ("p1", C.c_void_p), ("n1", C.c_void_p), ("n2", C.c_void_p),
        ("p2_stride", C.c_ssize_t), ("p1_stride", C.c_ssize_t), ("n1_stride", C.c_ssize_t), ("n2_stride", C.c_ssize_t),
    ]


class DebandCfg(C.Structure):
    """vszip_deband_cfg"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ssw", C.c_int32), ("ssh", C.c_int32), ("num_frames", C.c_int32), ("range", C.c_int32),
                ("sample_mode", C.c_int32), ("seed", C.c_int32), ("random_algo_ref", C.c_int32), ("random_algo_grain", C.c_int32),
                ("random_param_ref", C.c_double), ("random_param_grain", C.c_double), ("is_float", C.c_int32), ("dynamic_grain", C.c_int32),
                ("grain_u16", C.c_uint16 * 2), ("grain_f32", C.c_float * 2)]


class DebandSizes(C.Structure):
    """vszip_deband_sizes"""
    _fields_ = [("luma_pairs", C.c_size_t), ("chroma_pairs", C.c_size_t), ("grain_items", C.c_size_t), ("grain_offsets", C.c_size_t),
                ("chroma_w", C.c_int32), ("chroma_h", C.c_int32)]


class DebandPlane(C.Structure):
    """vszip_deband_plane"""
    _fields_ = [("offsets", C.c_void_p), ("offsets_pitch", C.c_ssize_t), ("grain", C.c_void_p), ("grain_pitch", C.c_ssize_t), ("ssw", C.c_int32), ("ssh", C.c_int32),
                ("thr", C.c_float), ("thr1", C.c_float), ("thr2", C.c_float), ("lo", C.c_float), ("hi", C.c_float)]


class BilateralDitherCfg(C.Structure):
    """vszip_bilateral_dither_cfg"""
    _fields_ = [("m", C.c_float), ("wmax", C.c_float), ("sum_w_min", C.c_float), ("K", C.c_int32), ("subsampled", C.c_int32)]


class BilateralDitherPlane(C.Structure):
    """vszip_bilateral_dither_plane"""
    _fields_ = [("radius", C.c_int32), ("m", C.c_float), ("wmax", C.c_float), ("sum_w_min", C.c_float), ("points", C.c_void_p), ("K", C.c_int32)]


class CompressTables(C.Structure):
    """struct vszip_compress_tables"""
    _fields_ = [("codec", C.c_int32), ("qmul", (C.c_int32 * 64) * 2), ("deq", (C.c_int32 * 64) * 2), ("dc_q", C.c_int32), ("dc_scale", C.c_int32)]

    def as_dict(self) -> dict:
        """the fields as tests/compress_ref.py tables() names them"""
        return dict(codec=int(self.codec), qmul=np.array(self.qmul, np.int32).reshape(2, 64), deq=np.array(self.deq, np.int32).reshape(2, 64), dc_q=int(self.dc_q),
                    dc_scale=int(self.dc_scale))


class PackRGBFrame(C.Structure):
    """vszip_pack_rgb_frame"""
    _fields_ = [("r", C.c_void_p), ("g", C.c_void_p), ("b", C.c_void_p), ("r_stride", C.c_ssize_t), ("g_stride", C.c_ssize_t), ("b_stride", C.c_ssize_t),
                ("dst", C.c_void_p), ("dst_stride", C.c_ssize_t), ("w", C.c_int32), ("h", C.c_int32)]


class DepthPlane(C.Structure):
    """vszip_depth_plane"""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_ssize_t), ("dst", C.c_void_p), ("dst_stride", C.c_ssize_t), ("w", C.c_int32), ("h", C.c_int32),
                ("chroma", C.c_int32)]


DEPTH_STRUCTS = {"vszip_depth_plane": DepthPlane}
DITHER_NONE, DITHER_ERROR_DIFFUSION = 0, 1


class ColorMapFrame(C.Structure):
    """vszip_color_map_frame"""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_ssize_t), ("r", C.c_void_p), ("g", C.c_void_p), ("b", C.c_void_p),
                ("r_stride", C.c_ssize_t), ("g_stride", C.c_ssize_t), ("b_stride", C.c_ssize_t), ("w", C.c_int32), ("h", C.c_int32)]


class ImageUnpackFrame(C.Structure):
    """vszip_image_unpack_frame"""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_ssize_t), ("p", C.c_void_p * 3), ("a", C.c_void_p), ("p_stride", C.c_ssize_t * 3), ("a_stride", C.c_ssize_t),
                ("w", C.c_int32), ("h", C.c_int32)]


IMG_GRAY, IMG_GRAY_ALPHA, IMG_RGB, IMG_RGBA, IMG_BGR, IMG_BGRA, IMG_INDEXED = range(7)


class BilateralCfg(C.Structure):
    _fields_ = [
        ("sigmaS", C.c_double), ("sigmaR", C.c_double), ("process", C.c_int32), ("algorithm", C.c_int32),
        ("pbficnum", C.c_int32), ("radius", C.c_int32), ("step", C.c_int32), ("samples", C.c_int32),
        ("gs_lut", C.c_void_p), ("gr_lut", C.c_void_p),
    ]


class ChainStage(C.Structure):
    """vszip_chain_stage"""
    _fields_ = [("kind", C.c_int32), ("process", C.c_int32 * 3), ("hradius", C.c_int32), ("hpasses", C.c_int32), ("vradius", C.c_int32), ("vpasses", C.c_int32),
                ("bilateral", C.POINTER(BilateralCfg) * 3), ("peak", C.c_float), ("lo", C.c_double * 3), ("hi", C.c_double * 3)]


STAGE_BOXBLUR, STAGE_BILATERAL, STAGE_LIMITER = 0, 1, 2
(STAGE_CLAHE, STAGE_COMB_MASK, STAGE_COMB_MASK_MT, STAGE_CHECKMATE, STAGE_MOSQUITO_NR, STAGE_DEBAND, STAGE_BILATERAL_DITHER,
 STAGE_COMPRESS) = range(3, 11)


class ChainOp(C.Structure):
    """vszip_chain_op"""
    _fields_ = [("kind", C.c_int32), ("process", C.c_int32 * 3), ("params", C.c_void_p)]


class ChainBoxBlur(C.Structure):
    """vszip_chain_boxblur"""
    _fields_ = [("hradius", C.c_int32), ("hpasses", C.c_int32), ("vradius", C.c_int32), ("vpasses", C.c_int32)]


class ChainBilateral(C.Structure):
    """vszip_chain_bilateral"""
    _fields_ = [("cfg", C.POINTER(BilateralCfg) * 3), ("peak", C.c_float)]


class ChainLimiter(C.Structure):
    """vszip_chain_limiter"""
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3)]


class ChainClahe(C.Structure):
    """vszip_chain_clahe"""
    _fields_ = [("limit", C.c_uint32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32)]


class ChainCombMask(C.Structure):
    """vszip_chain_comb_mask"""
    _fields_ = [("cthresh", C.c_int32), ("mthresh", C.c_int32), ("expand", C.c_int32), ("metric", C.c_int32)]


class ChainCombMaskMT(C.Structure):
    """vszip_chain_comb_mask_mt"""
    _fields_ = [("thy1", C.c_int32), ("thy2", C.c_int32)]


class ChainCheckmate(C.Structure):
    """vszip_chain_checkmate"""
    _fields_ = [("thr", C.c_int32), ("tmax", C.c_int32), ("tthr2", C.c_int32)]


class ChainMosquitoNR(C.Structure):
    """vszip_chain_mosquito_nr"""
    _fields_ = [("strength", C.POINTER(C.c_int32)), ("restore", C.POINTER(C.c_int32)), ("radius", C.POINTER(C.c_int32)), ("chroma", C.POINTER(C.c_uint8))]


class ChainDeband(C.Structure):
    """vszip_chain_deband"""
    _fields_ = [("per", C.POINTER(DebandPlane)), ("sample_mode", C.c_int32), ("blur_first", C.c_int32), ("angle_boost", C.c_float), ("max_angle", C.c_float),
                ("max_offset", C.c_int32)]


class ChainBilateralDither(C.Structure):
    """vszip_chain_bilateral_dither"""
    _fields_ = [("per", C.POINTER(BilateralDitherPlane))]


class ChainCompress(C.Structure):
    """vszip_chain_compress"""
    _fields_ = [("tables", C.POINTER(CompressTables)), ("chroma", C.POINTER(C.c_uint8))]


# C name -> ctypes class of every struct of vszip_chain_ops (tests/test_chain_plan_host.py compares sizes and offsets with the compiler's)
CHAIN_STRUCTS = {"vszip_chain_op": ChainOp, "vszip_chain_boxblur": ChainBoxBlur, "vszip_chain_bilateral": ChainBilateral, "vszip_chain_limiter": ChainLimiter,
                 "vszip_chain_clahe": ChainClahe, "vszip_chain_comb_mask": ChainCombMask, "vszip_chain_comb_mask_mt": ChainCombMaskMT,
                 "vszip_chain_checkmate": ChainCheckmate, "vszip_chain_mosquito_nr": ChainMosquitoNR, "vszip_chain_deband": ChainDeband,
                 "vszip_chain_bilateral_dither": ChainBilateralDither, "vszip_chain_compress": ChainCompress}


class SsimSource(C.Structure):
    """vszip_ssim_source: family (0 RGB, 1 Gray, 2 YUV), dtype, bits, limited, linearize; YUV: ssw, ssh, matrix, chroma_loc, chroma_stride."""
    _fields_ = [("family", C.c_int32), ("dtype", C.c_int32), ("bits", C.c_int32), ("limited", C.c_int32), ("linearize", C.c_int32),
                ("ssw", C.c_int32), ("ssh", C.c_int32), ("matrix", C.c_int32), ("chroma_loc", C.c_int32), ("chroma_stride", C.c_ssize_t)]


CF_RGB, CF_GRAY, CF_YUV = 0, 1, 2


class Eedi3Params(C.Structure):
    _fields_ = [("dh", C.c_int32), ("alpha", C.c_float), ("beta", C.c_float), ("gamma", C.c_float), ("nrad", C.c_int32), ("mdis", C.c_int32),
                ("hp", C.c_int32), ("vcheck", C.c_int32), ("vthresh0", C.c_float), ("vthresh1", C.c_float), ("vthresh2", C.c_float)]


# every symbol include/vszip_hip.h declares: name -> (restype, argtypes)
_vp, _i, _sz, _pd = C.c_void_p, C.c_int, C.c_size_t, C.c_ssize_t
_PP = C.POINTER(Plane)
SYMBOLS = {
    "vszip_abi_version": (_i, []),
    "vszip_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "vszip_ctx_destroy": (None, [_vp]),
    "vszip_ctx_set_stream": (_i, [_vp, _vp]),
    "vszip_ctx_stream": (_vp, [_vp]),
    "vszip_ctx_sync": (_i, [_vp]),
    "vszip_ctx_set_staging": (_i, [_vp, _i]),
    "vszip_ctx_abort": (_i, [_vp]),
    "vszip_ctx_set_option": (_i, [_vp, C.c_char_p, _i]),
    "vszip_ctx_get_option": (_i, [_vp, C.c_char_p, C.POINTER(_i)]),
    "vszip_dev_arena_info": (_i, [_vp, _vp, C.POINTER(_i), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vszip_dev_probe_region": (_i, [_vp, _vp, _sz, _vp, C.POINTER(C.c_double)]),
    "vszip_last_error": (C.c_char_p, [_vp]),
    "vszip_dev_alloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "vszip_dev_free": (_i, [_vp, _vp]),
    "vszip_dev_memset": (_i, [_vp, _vp, _i, _sz]),
    "vszip_host_alloc_pinned": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "vszip_host_free_pinned": (_i, [_vp, _vp]),
    "vszip_copy_h2d_2d": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "vszip_copy_d2h_2d": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "vszip_copy_d2d_2d": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "vszip_timer_start": (_i, [_vp]),
    "vszip_timer_stop_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "vszip_probe_enable": (_i, [_vp, _i]),
    "vszip_probe_read": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    "vszip_probe_read_each": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i), C.POINTER(C.c_float), _i]),
    "vszip_boxblur": (_i, [_vp, _i, _PP, _i, _i, _i, _i, _i]),
    "vszip_bilateral_derive": (_i, [C.POINTER(C.c_double), _i, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int), _i, _i, _i,
                                    C.POINTER(C.c_int), C.POINTER(BilateralCfg)]),
    "vszip_bilateral_luts": (_i, [_vp, C.POINTER(BilateralCfg), _i]),
    "vszip_bilateral": (_i, [_vp, _i, _PP, C.POINTER(C.POINTER(BilateralCfg)), _i, C.c_float]),
    "vszip_ssimulacra2": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _pd, _i, _i, _i, C.POINTER(C.c_double)]),
    "vszip_chain_run": (_i, [_vp, _i, C.POINTER(ChainStage), _i, _PP, C.POINTER(C.c_int), _i]),
    "vszip_chain_ops": (_i, [_vp, _i, _i, C.POINTER(ChainOp), _i, _PP, C.POINTER(C.c_int), C.POINTER(C.c_int), _i]),
    "vszip_resample_table": (_i, [_i, _i, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "vszip_ssimulacra2_src": (_i, [_vp, C.POINTER(SsimSource), C.POINTER(_vp), C.POINTER(_vp), _pd, _i, _i, _i, C.POINTER(C.c_double)]),
    "vszip_to_rgbs_linear": (_i, [_vp, C.POINTER(SsimSource), C.POINTER(_vp), _pd, C.POINTER(_vp), _pd, _i, _i]),
    "vszip_eedi3": (_i, [_vp, _PP, C.POINTER(_vp), C.POINTER(_pd), _i, _i, _i, C.POINTER(Eedi3Params)]),
    "vszip_eedi3_mclip": (_i, [_vp, _PP, C.POINTER(_vp), C.POINTER(_pd), C.POINTER(_vp), C.POINTER(_pd), _i, _i, _i, C.POINTER(Eedi3Params)]),
    "vszip_xpsnr_wsse": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_pd), _i, _i, C.c_uint, _i,
                              C.POINTER(C.c_uint64)]),
    "vszip_xpsnr_wsse_batch": (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), C.POINTER(_pd), _i, _i,
                                    C.c_uint, _i, C.POINTER(C.c_uint64)]),
    "vszip_xpsnr_value": (C.c_double, [C.c_uint64, C.c_uint64, C.c_uint64, _i]),
    "vszip_xpsnr_average": (C.c_double, [C.c_double, C.c_double, C.c_uint64, C.c_uint64, _i, C.c_uint64]),
    "vszip_limiter": (_i, [_vp, _i, _PP, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vszip_limit_filter": (_i, [_vp, _i, _PP, C.POINTER(_vp), C.POINTER(_pd), _i, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "vszip_adaptive_binarize": (_i, [_vp, _PP, _i, _i]),
    "vszip_clahe": (_i, [_vp, _i, _PP, _i, C.c_uint32, _i, _i]),
    "vszip_comb_mask": (_i, [_vp, _PP, _i, _i, _i, _i, _i]),
    "vszip_comb_mask_mt": (_i, [_vp, _PP, _i, _i, _i]),
    "vszip_checkmate": (_i, [_vp, _PP, C.POINTER(TemporalNbrs), _i, _i, _i, _i]),
    "vszip_mosquito_nr": (_i, [_vp, _i, _i, _PP, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]),
    "vszip_deband_tables": (_i, [C.POINTER(DebandCfg), C.POINTER(DebandSizes), _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32), C.c_char_p, _sz]),
    "vszip_deband": (_i, [_vp, _i, _PP, C.POINTER(DebandPlane), _i, _i, _i, C.c_float, C.c_float, _i]),
    "vszip_depth_check": (_i, [_i, _i, _i, _i, C.POINTER(DepthPlane), _i, C.c_char_p, _sz]),
    "vszip_depth": (_i, [_vp, C.POINTER(DepthPlane), _i, _i, _i, _i, _i]),
    "vszip_depth_fmt_check": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(DepthPlane), _i, C.c_char_p, _sz]),
    "vszip_depth_fmt": (_i, [_vp, C.POINTER(DepthPlane), _i, _i, _i, _i, _i, _i, _i]),
    "vszip_deband_lowbit": (_i, [_vp, _i, _i, _PP, C.POINTER(DebandPlane), _i, _i, _i, C.c_float, C.c_float, _i]),
    "vszip_bilateral_dither_derive": (_i, [_i, _i, _i, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(BilateralDitherCfg), C.c_char_p, _sz]),
    "vszip_bilateral_dither_points": (_i, [_i, C.c_float, _vp, _sz, C.POINTER(C.c_int32)]),
    "vszip_bilateral_dither": (_i, [_vp, _i, _i, _PP, C.POINTER(BilateralDitherPlane), _i]),
    "vszip_compress_tables": (_i, [_i, _i, _i, _i, C.POINTER(CompressTables), C.c_char_p, _sz]),
    "vszip_compress": (_i, [_vp, _PP, _i, C.POINTER(CompressTables), C.POINTER(C.c_uint8)]),
    "vszip_pack_rgb": (_i, [_vp, _i, C.POINTER(PackRGBFrame), _i]),
    "vszip_color_map_lut": (_i, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), _i, _vp, C.c_char_p, _sz]),
    "vszip_color_map": (_i, [_vp, C.POINTER(ColorMapFrame), _i, _vp]),
    "vszip_image_unpack": (_i, [_vp, _i, _i, _i, C.POINTER(ImageUnpackFrame), _i, _vp]),
    "vszip_plane_average": (_i, [_vp, _i, _PP, _i, C.POINTER(C.c_int32), _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vszip_plane_minmax": (_i, [_vp, _i, _PP, _i, C.c_float, C.c_float, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vszip_plane_average_async": (_i, [_vp, _i, _PP, _i, C.POINTER(C.c_int32), _i, _i, _vp]),
    "vszip_plane_minmax_async": (_i, [_vp, _i, _PP, _i, C.c_float, C.c_float, _i, _vp]),
}

_lib = None


def resample_table(src_dim: int, dst_dim: int, shift: float = 0.0):
    """vszip_resample_table (device-free): zimg's Catmull-Rom upscale table of one axis -> (left[dst_dim] int32, coef[dst_dim, 4] f32)."""
    left = np.empty(dst_dim, np.int32)
    coef = np.empty((dst_dim, 4), np.float32)
    rc = load().vszip_resample_table(src_dim, dst_dim, float(shift), left.ctypes.data_as(C.POINTER(C.c_int32)), coef.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ValueError(f"vszip_resample_table({src_dim}, {dst_dim}, {shift}) -> {rc}")
    return left, coef


def depth_check(bits_in, bits_out, dither, full_range, planes) -> None:
    """vszip_depth_check (device-free): the argument checks of vszip_depth; planes: (src, src_stride, dst, dst_stride, w, h, chroma) tuples of plain
    integers (pointers are only compared with NULL). VszipError with the library's code and text."""
    n = len(planes)
    arr = (DepthPlane * max(n, 1))(*[DepthPlane(*p) for p in planes])
    err = C.create_string_buffer(256)
    rc = load().vszip_depth_check(int(bits_in), int(bits_out), int(dither), int(full_range), arr if n else None, n, err, len(err))
    if rc != 0:
        raise VszipError(rc, err.value.decode())


def depth_fmt_check(dtype_in, bits_in, dtype_out, bits_out, dither, full_range, planes) -> None:
    """vszip_depth_fmt_check (device-free): the argument checks of vszip_depth_fmt; dtypes U8 / U16 / F16 / F32, planes as for depth_check.
    VszipError with the library's code and text."""
    n = len(planes)
    arr = (DepthPlane * max(n, 1))(*[DepthPlane(*p) for p in planes])
    err = C.create_string_buffer(256)
    rc = load().vszip_depth_fmt_check(int(dtype_in), int(bits_in), int(dtype_out), int(bits_out), int(dither), int(full_range), arr if n else None, n, err, len(err))
    if rc != 0:
        raise VszipError(rc, err.value.decode())


def deband_tables(width, height, ssw=0, ssh=0, num_frames=1, range=15, sample_mode=2, seed=0, random_algo_ref=1, random_algo_grain=1, random_param_ref=1.0,
                  random_param_grain=1.0, grain=(0, 0), dynamic_grain=False, is_float=False) -> dict:
    """vszip_deband_tables (device-free): the per-clip tables of vszip.Deband as numpy arrays. grain: the luma and chroma strengths on the
    clip's scale (16-bit integers, or f32). -> luma (h, w, 2) int8, chroma (ch, cw, 2) int8, grain_y / grain_c (int16 | f32, None for
    strength 0), grain_offsets (uint32 per frame, None for static grain), max_offset, items (grain values of one frame).
    ValueError with the reference's wording for an argument out of range."""
    cfg = DebandCfg(int(width), int(height), int(ssw), int(ssh), int(num_frames), int(range), int(sample_mode), C.c_int32(int(seed) & 0xFFFFFFFF).value,
                    int(random_algo_ref), int(random_algo_grain), float(random_param_ref), float(random_param_grain), int(bool(is_float)), int(bool(dynamic_grain)))
    for i in (0, 1):
        if is_float:
            cfg.grain_f32[i] = float(grain[i])
        else:
            cfg.grain_u16[i] = int(grain[i])
    lib, sizes, err = load(), DebandSizes(), C.create_string_buffer(256)
    rc = lib.vszip_deband_tables(C.byref(cfg), C.byref(sizes), None, None, None, None, None, None, err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode() or f"vszip_deband_tables -> {rc}")
    luma = np.empty((int(height), int(width), 2), np.int8)
    chroma = np.empty((sizes.chroma_h, sizes.chroma_w, 2), np.int8)
    gt = np.float32 if is_float else np.int16
    gy = np.empty(sizes.grain_items, gt) if grain[0] > 0 else None
    gc = np.empty(sizes.grain_items, gt) if grain[1] > 0 else None
    offs = np.empty(sizes.grain_offsets, np.uint32) if sizes.grain_offsets else None
    mx = C.c_int32()
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = lib.vszip_deband_tables(C.byref(cfg), C.byref(sizes), ptr(luma), ptr(chroma), ptr(gy), ptr(gc), ptr(offs), C.byref(mx), err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode() or f"vszip_deband_tables -> {rc}")
    return dict(luma=luma, chroma=chroma, grain_y=gy, grain_c=gc, grain_offsets=offs, max_offset=mx.value, items=sizes.grain_items // (3 if dynamic_grain else 1))


def bilateral_dither_params(is_float, bits, radius=16, thr=2.5, flat=0.4, wmin=0.0, subspl=0.0) -> dict:
    """vszip_bilateral_dither_derive (device-free): one plane's wrapper arguments -> m, wmax, sum_w_min (np.float32), K (0: the dense window) and
    subsampled. ValueError with the reference's wording for an argument out of range."""
    cfg, err = BilateralDitherCfg(), C.create_string_buffer(256)
    rc = load().vszip_bilateral_dither_derive(int(bool(is_float)), int(bits), int(radius), float(thr), float(flat), float(wmin), float(subspl), C.byref(cfg), err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode() or f"vszip_bilateral_dither_derive -> {rc}")
    return dict(m=np.float32(cfg.m), wmax=np.float32(cfg.wmax), sum_w_min=np.float32(cfg.sum_w_min), K=int(cfg.K), subsampled=bool(cfg.subsampled))


def bilateral_dither_points(radius, subspl=0.0) -> np.ndarray:
    """vszip_bilateral_dither_points (device-free): the 23 point lists of a geometry as a (23, K, 2) int16 array, [..., 0] = x, [..., 1] = y"""
    lib, k = load(), C.c_int32()
    rc = lib.vszip_bilateral_dither_points(int(radius), float(subspl), None, 0, C.byref(k))
    if rc != 0:
        raise ValueError(f"vszip_bilateral_dither_points({radius}, {subspl}) -> {rc}")
    pts = np.empty((23, k.value, 2), np.int16)
    rc = lib.vszip_bilateral_dither_points(int(radius), float(subspl), pts.ctypes.data, 23 * k.value, C.byref(k))
    if rc != 0:
        raise ValueError(f"vszip_bilateral_dither_points({radius}, {subspl}) -> {rc}")
    return pts


def compress_tables(codec=0, qscale=8, dc_prec=0, quality=50) -> CompressTables:
    """vszip_compress_tables (device-free): the quantiser tables of vszip.Compress for one clip (codec 0 mpeg2 with qscale and dc_prec, 1 jpeg
    with quality). ValueError with the reference's wording for an argument out of range."""
    tb, err = CompressTables(), C.create_string_buffer(256)
    rc = load().vszip_compress_tables(int(codec), int(qscale), int(dc_prec), int(quality), C.byref(tb), err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode() or f"vszip_compress_tables -> {rc}")
    return tb


def color_map_lut(r, g, b) -> np.ndarray:
    """vszip_color_map_lut (device-free): a palette of len(r) points a channel (f32, 0..1) -> the (3, 256) uint8 table of vszip.ColorMap,
    interpolated and rounded as the reference's create function does. VszipError (VSZIP_ERR_ARG) naming the channel and the index for an empty
    palette and for an entry that is NaN or lands outside 0..255."""
    pal = [np.ascontiguousarray(c, np.float32).reshape(-1) for c in (r, g, b)]
    if not (len(pal[0]) == len(pal[1]) == len(pal[2])):
        raise ValueError("color_map_lut: r, g and b have one length")
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    lut, err = np.zeros((3, 256), np.uint8), C.create_string_buffer(256)
    rc = load().vszip_color_map_lut(fp(pal[0]), fp(pal[1]), fp(pal[2]), len(pal[0]), lut.ctypes.data, err, len(err))
    if rc != 0:
        raise VszipError(rc, err.value.decode() or f"vszip_color_map_lut -> {rc}")
    return lut


def _share_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so.7 (same soname as the system one). Two HIP
    runtimes in one process do not work (the second finds no device), and whichever is loaded
    first wins the soname: when torch is installed but not imported yet, load ITS runtime first, so
    that libvszip_hip.so and a later `import torch` share one — the same state as importing torch
    before this module. Without torch installed the system runtime is used."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")  # does not import torch
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    cand = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
    if cand.is_file():
        C.CDLL(str(cand), mode=C.RTLD_GLOBAL)


def load() -> C.CDLL:
    """dlopen libvszip_hip.so and declare every exported entry point."""
    global _lib
    if _lib is None:
        if not LIB_PATH.is_file():
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python vapoursynth-zip_amd/build.py` "
                "(there is no CPU fallback)"
            )
        _share_torch_hip_runtime()
        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class DevPlane:
    """A 2-D plane in device memory with a row pitch (in elements)."""

    __slots__ = ("dev", "ptr", "w", "h", "stride", "dtype", "_own")

    def __init__(self, dev: "Device", ptr: int, w: int, h: int, stride: int, dtype, own: bool = True):
        self.dev, self.ptr, self.w, self.h, self.stride, self.dtype, self._own = dev, ptr, w, h, stride, np.dtype(dtype), own

    @property
    def nbytes(self) -> int:
        return self.stride * self.h * self.dtype.itemsize

    def free(self):
        if self._own and self.ptr:
            self.dev.lib.vszip_dev_free(self.dev.ctx, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Device:
    """One context (GPU + stream)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        ctx = C.c_void_p()
        rc = self.lib.vszip_ctx_create(device, C.byref(ctx))
        if rc != OK:
            raise VszipError(rc, f"vszip_ctx_create(device={device}) failed with {rc} (no MI355X visible?)")
        self.ctx = ctx
        self.device = device

    def close(self):
        if self.ctx:
            for hp in getattr(self, "_pinned", []):
                self.lib.vszip_host_free_pinned(self.ctx, C.c_void_p(hp))
            self._pinned = []
            self.lib.vszip_ctx_destroy(self.ctx)
            self.ctx = None

    def check(self, rc: int):
        if rc != OK:
            raise VszipError(rc, self.lib.vszip_last_error(self.ctx).decode())

    def sync(self):
        self.check(self.lib.vszip_ctx_sync(self.ctx))

    def set_staging(self, mode: int):
        """0: host copies go straight from/to the caller's memory; 1: through the context's pinned arena."""
        self.check(self.lib.vszip_ctx_set_staging(self.ctx, mode))

    def set_option(self, name: str, value: int = 1):
        """vszip_ctx_set_option: one switch of csrc/options.inc on this context, by its environment name.
        VszipError with code VSZIP_ERR_UNSUPPORTED for a development variant a default build does not contain."""
        saved = self.__dict__.setdefault("_opt_saved", {})
        if name not in saved:
            try:
                saved[name] = self.get_option(name)
            except VszipError:
                pass
        self.check(self.lib.vszip_ctx_set_option(self.ctx, name.encode(), int(value)))

    def restore_options(self, keep=()):
        """every option set through set_option back to its value before the first set (tests)"""
        for k, v in list(self.__dict__.get("_opt_saved", {}).items()):
            if k not in keep:
                self.lib.vszip_ctx_set_option(self.ctx, k.encode(), int(v))
                del self._opt_saved[k]

    def get_option(self, name: str) -> int:
        v = C.c_int()
        self.check(self.lib.vszip_ctx_get_option(self.ctx, name.encode(), C.byref(v)))
        return v.value

    def variant(self, **kw):
        """like options(), for switches that may be development variants: yields False (and sets nothing) when this build does not
        contain them (VSZIP_ERR_UNSUPPORTED), so a path-agreement test compares the alternative only where it exists"""
        import contextlib

        @contextlib.contextmanager
        def scope():
            try:
                for k in kw:
                    self.get_option(k)
            except VszipError as e:
                if e.code != -3:
                    raise
                for k in kw:  # counted: tests/conftest.py reports how many cross-checks a default build left out
                    VARIANTS_ABSENT[k] = VARIANTS_ABSENT.get(k, 0) + 1
                yield False
                return
            with self.options(**kw):
                yield True

        return scope()

    def options(self, **kw):
        """`with dev.options(VSZIP_RT_NO_ICHAIN=1): ...` — set, run, restore (the path-agreement tests)"""
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = {k: self.get_option(k) for k in kw}
            try:
                for k, v in kw.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)

        return scope()

    def arena_info(self, ptr: int) -> dict:
        """vszip_dev_arena_info: what the placement search did for a vszip_dev_alloc pointer (candidates = 0: a plain allocation)"""
        nc, rate, ms = C.c_int(), C.c_double(), C.c_double()
        self.check(self.lib.vszip_dev_arena_info(self.ctx, C.c_void_p(ptr), C.byref(nc), C.byref(rate), C.byref(ms)))
        return {"candidates": nc.value, "probe_bytes_per_second": rate.value, "search_ms": ms.value}

    def probe_region(self, ptr: int, nbytes: int, src: int = 0) -> float:
        bps = C.c_double()
        self.check(self.lib.vszip_dev_probe_region(self.ctx, C.c_void_p(ptr), nbytes, C.c_void_p(src) if src else None, C.byref(bps)))
        return bps.value

    def set_stream(self, hip_stream: int):
        """Enqueue on an externally owned hipStream_t (e.g. torch.cuda.Stream().cuda_stream)."""
        self.check(self.lib.vszip_ctx_set_stream(self.ctx, C.c_void_p(hip_stream)))

    def wrap(self, ptr: int, h: int, w: int, stride: int, dtype) -> "DevPlane":
        """A DevPlane view of device memory this context does not own (e.g. a torch tensor's data_ptr)."""
        return DevPlane(self, ptr, w, h, stride, np.dtype(dtype), own=False)

    # -- memory ---------------------------------------------------------------
    def empty(self, h: int, w: int, dtype, align_elems: int = 32) -> DevPlane:
        dtype = np.dtype(dtype)
        stride = -(-w // align_elems) * align_elems
        p = C.c_void_p()
        # The + 256 is slack behind the last row that dates from the first kernel commit: a read that ran up to 256 bytes past a plane would land in it
        # unseen. It is not part of the contract (include/vszip_hip.h, "Plane memory": a caller owns h x stride samples and no more) and nothing may
        # rely on it; what keeps kernels inside their planes is tests/test_gpu_footprint.py, whose planes do not come from here (tests/guarded.py).
        self.check(self.lib.vszip_dev_alloc(self.ctx, stride * h * dtype.itemsize + 256, C.byref(p)))
        return DevPlane(self, p.value, w, h, stride, dtype)

    def upload(self, a: np.ndarray, align_elems: int = 32) -> DevPlane:
        assert a.ndim == 2 and a.strides[1] == a.itemsize
        d = self.empty(a.shape[0], a.shape[1], a.dtype, align_elems)
        self.check(self.lib.vszip_copy_h2d_2d(self.ctx, d.ptr, d.stride * a.itemsize, a.ctypes.data, a.strides[0], a.shape[1] * a.itemsize, a.shape[0]))
        self.sync()
        return d

    def pinned_array(self, shape, dtype) -> np.ndarray:
        """Host array in page-locked memory (async copies; what a plugin keeps per worker)."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self.check(self.lib.vszip_host_alloc_pinned(self.ctx, n, C.byref(p)))
        buf = (C.c_char * n).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", []) + [p.value]
        return a

    def copy_in(self, d: DevPlane, a: np.ndarray):
        """Async H2D of a host array into an existing device plane (no synchronisation)."""
        self.check(self.lib.vszip_copy_h2d_2d(self.ctx, d.ptr, d.stride * a.itemsize, a.ctypes.data, a.strides[0], a.shape[1] * a.itemsize, a.shape[0]))

    def copy_out(self, a: np.ndarray, d: DevPlane):
        """Async D2H of a device plane into a host array (no synchronisation)."""
        self.check(self.lib.vszip_copy_d2h_2d(self.ctx, a.ctypes.data, a.strides[0], d.ptr, d.stride * d.dtype.itemsize, d.w * d.dtype.itemsize, d.h))

    def download(self, d: DevPlane) -> np.ndarray:
        out = np.empty((d.h, d.w), dtype=d.dtype)
        self.check(self.lib.vszip_copy_d2h_2d(self.ctx, out.ctypes.data, out.strides[0], d.ptr, d.stride * d.dtype.itemsize, d.w * d.dtype.itemsize, d.h))
        self.sync()
        return out

    # -- timing ---------------------------------------------------------------
    def timer_start(self):
        self.check(self.lib.vszip_timer_start(self.ctx))

    def probe_enable(self, on: bool):
        self.check(self.lib.vszip_probe_enable(self.ctx, int(on)))

    def probe_read(self):
        """(summed dominant-kernel ms, launches) since the probe was enabled / last read."""
        ms, n = C.c_double(), C.c_int()
        self.check(self.lib.vszip_probe_read(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def probe_read_each(self, cap: int = 65536):
        """(summed ms, launches, [per-launch ms]) — the per-launch durations in launch order."""
        ms, n = C.c_double(), C.c_int()
        each = (C.c_float * cap)()
        self.check(self.lib.vszip_probe_read_each(self.ctx, C.byref(ms), C.byref(n), each, cap))
        return ms.value, n.value, [each[i] for i in range(min(n.value, cap))]

    def timer_stop_ms(self) -> float:
        ms = C.c_float()
        self.check(self.lib.vszip_timer_stop_ms(self.ctx, C.byref(ms)))
        return ms.value

    # -- filters --------------------------------------------------------------
    @staticmethod
    def plane_table(srcs, dsts=None, refs=None):
        n = len(srcs)
        arr = (Plane * n)()
        for i, s in enumerate(srcs):
            arr[i].src, arr[i].src_stride, arr[i].w, arr[i].h = s.ptr, s.stride, s.w, s.h
            if dsts is not None:
                arr[i].dst, arr[i].dst_stride = dsts[i].ptr, dsts[i].stride
            if refs is not None and refs[i] is not None:
                arr[i].ref, arr[i].ref_stride = refs[i].ptr, refs[i].stride
        return arr

    def boxblur_table(self, dtype, table, hradius=1, hpasses=1, vradius=1, vpasses=1):
        self.check(self.lib.vszip_boxblur(self.ctx, _NP2DT[np.dtype(dtype)], table, len(table), hradius, hpasses, vradius, vpasses))

    def boxblur(self, srcs, dsts, hradius=1, hpasses=1, vradius=1, vpasses=1):
        self.boxblur_table(srcs[0].dtype, self.plane_table(srcs, dsts), hradius, hpasses, vradius, vpasses)

    def plane_average(self, srcs, exclude=(), refs=None, bits=None):
        """-> (avg[], diff[] or None) for a list of planes of one sample type."""
        n = len(srcs)
        table = self.plane_table(srcs, None, refs)
        ex = (C.c_int32 * max(1, len(exclude)))(*exclude)
        avg, diff = (C.c_double * n)(), (C.c_double * n)()
        b = bits if bits is not None else 8 * srcs[0].dtype.itemsize
        self.check(self.lib.vszip_plane_average(self.ctx, _NP2DT[srcs[0].dtype], table, n, ex, len(exclude), b, avg, diff))
        return list(avg), (list(diff) if refs is not None else None)

    def plane_average_async(self, srcs, results, exclude=(), refs=None, bits=None):
        """vszip_plane_average_async: `results` is a pinned_array((len(srcs), 4), float64); valid after the next sync()"""
        n = len(srcs)
        table = self.plane_table(srcs, None, refs)
        ex = (C.c_int32 * max(1, len(exclude)))(*exclude)
        b = bits if bits is not None else 8 * srcs[0].dtype.itemsize
        self.check(self.lib.vszip_plane_average_async(self.ctx, _NP2DT[srcs[0].dtype], table, n, ex, len(exclude), b, results.ctypes.data))

    def plane_minmax_async(self, srcs, results, minthr=0.0, maxthr=0.0, refs=None, bits=None):
        """vszip_plane_minmax_async: results[i] = (min, max, diff, -), pinned; valid after the next sync()"""
        n = len(srcs)
        table = self.plane_table(srcs, None, refs)
        b = bits if bits is not None else 8 * srcs[0].dtype.itemsize
        self.check(self.lib.vszip_plane_minmax_async(self.ctx, _NP2DT[srcs[0].dtype], table, n, minthr, maxthr, b, results.ctypes.data))

    def limiter(self, srcs, dsts, lo, hi):
        """dsts[i] = min(max(lo[i], srcs[i]), hi[i]) (vszip.Limiter with the bounds already resolved)."""
        n = len(srcs)
        table = self.plane_table(srcs, dsts)
        self.check(self.lib.vszip_limiter(self.ctx, _NP2DT[srcs[0].dtype], table, n, (C.c_double * n)(*[float(v) for v in lo]), (C.c_double * n)(*[float(v) for v in hi])))

    def prepared_limiter(self, srcs, dsts, lo, hi):
        """-> a callable queueing vszip_limiter on argument blocks built once."""
        n = len(srcs)
        table = self.plane_table(srcs, dsts)
        los, his = (C.c_double * n)(*[float(v) for v in lo]), (C.c_double * n)(*[float(v) for v in hi])
        dt, fn, ctx, check = _NP2DT[srcs[0].dtype], self.lib.vszip_limiter, self.ctx, self.check
        return lambda: check(fn(ctx, dt, table, n, los, his))

    @staticmethod
    def clahe_tiles(tiles) -> tuple:
        """the wrapper's `tiles` argument (src/vapoursynth/clahe.zig:76-91): an int, [n] or [x, y] -> (tiles_x, tiles_y)"""
        t = [int(tiles)] if isinstance(tiles, (int, np.integer)) else [int(v) for v in tiles]
        if len(t) < 1 or len(t) > 2:
            raise ValueError("CLAHE : tiles array can't have more than 2 values.")
        return (t[0], t[1] if len(t) == 2 else t[0])

    def clahe(self, srcs, dsts, limit=7, tiles=3):
        """vszip.CLAHE on every plane of srcs (8- or 16-bit, any sizes; dsts may be srcs): limit, tiles as the reference's defaults."""
        tx, ty = self.clahe_tiles(tiles)
        table = self.plane_table(srcs, dsts)
        self.check(self.lib.vszip_clahe(self.ctx, _NP2DT[srcs[0].dtype], table, len(srcs), int(limit), tx, ty))

    def prepared_clahe(self, srcs, dsts, limit=7, tiles=3):
        """-> a callable queueing vszip_clahe on argument blocks built once."""
        tx, ty = self.clahe_tiles(tiles)
        n = len(srcs)
        table = self.plane_table(srcs, dsts)
        dt, fn, ctx, check, lim = _NP2DT[srcs[0].dtype], self.lib.vszip_clahe, self.ctx, self.check, int(limit)
        return lambda: check(fn(ctx, dt, table, n, lim, tx, ty))

    def comb_mask(self, srcs, dsts, prevs=None, cthresh=6, mthresh=9, expand=True, metric=0):
        """vszip.CombMask on every plane of srcs (u8, any sizes, at least 3 rows): dsts[i] = 255 / 0. prevs[i]: the same plane of the
        previous frame (frame 0: srcs[i] itself), needed when mthresh > 0."""
        table = self.plane_table(srcs, dsts, prevs)
        self.check(self.lib.vszip_comb_mask(self.ctx, table, len(srcs), int(cthresh), int(mthresh), int(bool(expand)), int(metric)))

    def prepared_comb_mask(self, srcs, dsts, prevs=None, cthresh=6, mthresh=9, expand=True, metric=0):
        """-> a callable queueing vszip_comb_mask on argument blocks built once."""
        n = len(srcs)
        table = self.plane_table(srcs, dsts, prevs)
        fn, ctx, check, args = self.lib.vszip_comb_mask, self.ctx, self.check, (int(cthresh), int(mthresh), int(bool(expand)), int(metric))
        return lambda: check(fn(ctx, table, n, *args))

    def comb_mask_mt(self, srcs, dsts, thY1=30, thY2=30):
        """vszip.CombMaskMT on every plane of srcs (u8, at least 3 rows)."""
        self.check(self.lib.vszip_comb_mask_mt(self.ctx, self.plane_table(srcs, dsts), len(srcs), int(thY1), int(thY2)))

    def prepared_comb_mask_mt(self, srcs, dsts, thY1=30, thY2=30):
        """-> a callable queueing vszip_comb_mask_mt on argument blocks built once."""
        n = len(srcs)
        table = self.plane_table(srcs, dsts)
        fn, ctx, check, a, b = self.lib.vszip_comb_mask_mt, self.ctx, self.check, int(thY1), int(thY2)
        return lambda: check(fn(ctx, table, n, a, b))

    @staticmethod
    def temporal_nbrs(p1s, n1s, p2s=None, n2s=None):
        """-> the vszip_temporal_nbrs array of a plane table: the same plane of frames n - 1, n + 1 (and n - 2, n + 2), already clamped"""
        arr = (TemporalNbrs * len(p1s))()
        for i in range(len(p1s)):
            arr[i].p1, arr[i].p1_stride, arr[i].n1, arr[i].n1_stride = p1s[i].ptr, p1s[i].stride, n1s[i].ptr, n1s[i].stride
            if p2s is not None and p2s[i] is not None:
                arr[i].p2, arr[i].p2_stride = p2s[i].ptr, p2s[i].stride
            if n2s is not None and n2s[i] is not None:
                arr[i].n2, arr[i].n2_stride = n2s[i].ptr, n2s[i].stride
        return arr

    def checkmate(self, srcs, dsts, p1s, n1s, p2s=None, n2s=None, thr=12, tmax=12, tthr2=0):
        """vszip.Checkmate on every plane of srcs (u8, any sizes, at least 3 x 5): p1s / n1s (and, for tthr2 > 0, p2s / n2s) are the same
        planes of the neighbouring frames, clamped to the clip (they may be srcs[i] itself)."""
        self.check(self.lib.vszip_checkmate(self.ctx, self.plane_table(srcs, dsts), self.temporal_nbrs(p1s, n1s, p2s, n2s), len(srcs), int(thr), int(tmax), int(tthr2)))

    def prepared_checkmate(self, srcs, dsts, p1s, n1s, p2s=None, n2s=None, thr=12, tmax=12, tthr2=0):
        """-> a callable queueing vszip_checkmate on argument blocks built once."""
        n = len(srcs)
        table, nbrs = self.plane_table(srcs, dsts), self.temporal_nbrs(p1s, n1s, p2s, n2s)
        fn, ctx, check, args = self.lib.vszip_checkmate, self.ctx, self.check, (int(thr), int(tmax), int(tthr2))
        return lambda: check(fn(ctx, table, nbrs, n, *args))

    @staticmethod
    def clip_neighbours(frames):
        """frames[f]: the planes of frame f -> flat (srcs, p1s, n1s, p2s, n2s) over all planes of the clip, frame indices clamped as the
        wrapper's getFrame does: max(0, n - k), min(n + k, frames - 1)"""
        last = len(frames) - 1
        pick = lambda off: [p for f in range(len(frames)) for p in frames[min(max(f + off, 0), last)]]
        return pick(0), pick(-1), pick(1), pick(-2), pick(2)

    def prepared_checkmate_clip(self, frames, dsts, thr=12, tmax=12, tthr2=0):
        """-> a callable queueing checkmate_clip on argument blocks built once."""
        srcs, p1s, n1s, p2s, n2s = self.clip_neighbours(frames)
        return self.prepared_checkmate(srcs, [p for f in dsts for p in f], p1s, n1s, p2s, n2s, thr, tmax, tthr2)

    def checkmate_clip(self, frames, dsts, thr=12, tmax=12, tthr2=0):
        """vszip.Checkmate on a whole resident clip: frames[f] / dsts[f] are the device planes of frame f. One vszip_checkmate over
        all planes of the clip; a frame's neighbours are the clip's other frames (nothing is copied)."""
        self.prepared_checkmate_clip(frames, dsts, thr, tmax, tthr2)()

    def _mosquito_args(self, srcs, dsts, strength, restore, radius, bits, chroma):
        n = len(srcs)
        per = lambda v: [int(v)] * n if isinstance(v, (int, np.integer)) else [int(x) for x in v]
        st, rs, rd = per(strength), per(restore), per(radius)
        if not (len(st) == len(rs) == len(rd) == n):
            raise ValueError("mosquito_nr: strength, restore and radius are scalars or one value per plane")
        dt = srcs[0].dtype
        b = int(bits) if bits is not None else 8 * dt.itemsize
        i32 = lambda v: (C.c_int32 * n)(*v)
        ch = None
        if chroma is not None:
            ch = (C.c_uint8 * n)(*([int(bool(chroma))] * n if isinstance(chroma, (bool, int, np.integer)) else [int(bool(c)) for c in chroma]))
        return (_NP2DT[dt], b, self.plane_table(srcs, dsts), n, i32(st), i32(rs), i32(rd), ch)

    def mosquito_nr(self, srcs, dsts, strength=16, restore=128, radius=2, bits=None, chroma=None):
        """vszip.MosquitoNR on every plane of srcs (u8, u16 with `bits` 9 .. 16, or f32; any sizes from 4 x 4): strength, restore and
        radius are scalars or one value per plane; chroma (float planes: the clamp is [-0.5, 0.5]) likewise, None = all luma. Planes
        with strength 0 are copied. dsts must not overlap srcs."""
        self.check(self.lib.vszip_mosquito_nr(self.ctx, *self._mosquito_args(srcs, dsts, strength, restore, radius, bits, chroma)))

    def prepared_mosquito_nr(self, srcs, dsts, strength=16, restore=128, radius=2, bits=None, chroma=None):
        """-> a callable queueing vszip_mosquito_nr on argument blocks built once."""
        fn, ctx, check, args = self.lib.vszip_mosquito_nr, self.ctx, self.check, self._mosquito_args(srcs, dsts, strength, restore, radius, bits, chroma)
        return lambda: check(fn(ctx, *args))

    def _compress_args(self, srcs, dsts, tables, chroma):
        n = len(srcs)
        if len(dsts) != n or any(s.dtype != np.uint8 for s in srcs):
            raise ValueError("compress: one destination per plane, 8-bit planes only")
        ch = None
        if chroma is not None:
            ch = (C.c_uint8 * n)(*([int(bool(chroma))] * n if isinstance(chroma, (bool, int, np.integer)) else [int(bool(c)) for c in chroma]))
            if len(ch) != n:
                raise ValueError("compress: chroma is a scalar or one value per plane")
        return (self.plane_table(srcs, dsts), n, C.byref(tables) if tables is not None else None, ch)

    def compress(self, srcs, dsts, tables, chroma=None):
        """vszip.Compress on every plane of srcs (u8, any sizes): tables from compress_tables(); chroma a scalar or one value per plane
        (true: the chroma tables), None = all luma. dsts[i] may be srcs[i] itself."""
        self.check(self.lib.vszip_compress(self.ctx, *self._compress_args(srcs, dsts, tables, chroma)))

    def prepared_compress(self, srcs, dsts, tables, chroma=None):
        """-> a callable queueing vszip_compress on argument blocks built once."""
        fn, ctx, check, args = self.lib.vszip_compress, self.ctx, self.check, self._compress_args(srcs, dsts, tables, chroma)
        return lambda: check(fn(ctx, *args))

    def _pack_rgb_args(self, rs, gs, bs, dsts, bits):
        n = len(rs)
        if not (len(gs) == len(bs) == len(dsts) == n):
            raise ValueError("pack_rgb: one g, b and dst plane per r plane")
        want = {8: np.uint8, 10: np.uint16}.get(int(bits))
        if want is not None and any(p.dtype != want for p in (*rs, *gs, *bs)):
            raise ValueError(f"pack_rgb: bits={bits} takes {np.dtype(want).name} planes")
        if any(d.dtype != np.uint32 for d in dsts):
            raise ValueError("pack_rgb: dst planes are uint32")
        arr = (PackRGBFrame * n)()
        for i in range(n):
            arr[i] = PackRGBFrame(rs[i].ptr, gs[i].ptr, bs[i].ptr, rs[i].stride, gs[i].stride, bs[i].stride, dsts[i].ptr, dsts[i].stride, dsts[i].w, dsts[i].h)
        return (int(bits), arr, n)

    def pack_rgb(self, rs, gs, bs, dsts, bits=8):
        """vszip.PackRGB on every frame: rs / gs / bs the planes of RGB24 (u8, bits=8) or RGB30 (u16, bits=10), dsts the packed u32 planes
        (b | g << 8 | r << 16 | 255 << 24, or b | g << 10 | r << 20 | 3 << 30); any mix of sizes. The inputs may alias each other."""
        self.check(self.lib.vszip_pack_rgb(self.ctx, *self._pack_rgb_args(rs, gs, bs, dsts, bits)))

    def prepared_pack_rgb(self, rs, gs, bs, dsts, bits=8):
        """-> a callable queueing vszip_pack_rgb on argument blocks built once."""
        fn, ctx, check, args = self.lib.vszip_pack_rgb, self.ctx, self.check, self._pack_rgb_args(rs, gs, bs, dsts, bits)
        return lambda: check(fn(ctx, *args))

    def _color_map_args(self, srcs, rs, gs, bs, lut):
        n = len(srcs)
        if not (len(rs) == len(gs) == len(bs) == n) or any(p.dtype != np.uint8 for p in (*srcs, *rs, *gs, *bs)):
            raise ValueError("color_map: one r, g and b plane per source plane, 8-bit planes only")
        if lut is not None and (not isinstance(lut, np.ndarray) or lut.dtype != np.uint8 or lut.shape != (3, 256) or not lut.flags.c_contiguous):
            raise ValueError("color_map: lut is a C-contiguous (3, 256) uint8 array (color_map_lut)")
        arr = (ColorMapFrame * n)()
        for i in range(n):
            arr[i] = ColorMapFrame(srcs[i].ptr, srcs[i].stride, rs[i].ptr, gs[i].ptr, bs[i].ptr, rs[i].stride, gs[i].stride, bs[i].stride, srcs[i].w, srcs[i].h)
        return (arr, n, lut)

    def color_map(self, srcs, rs, gs, bs, lut):
        """vszip.ColorMap on every frame: srcs Gray8 planes, rs / gs / bs the planes of the RGB24 result, lut the (3, 256) uint8 table of
        color_map_lut() (consumed before the call returns); any mix of sizes."""
        arr, n, lut = self._color_map_args(srcs, rs, gs, bs, lut)
        self.check(self.lib.vszip_color_map(self.ctx, arr, n, lut.ctypes.data if lut is not None else None))

    def prepared_color_map(self, srcs, rs, gs, bs, lut):
        """-> a callable queueing vszip_color_map on argument blocks built once (the table is read at every call)."""
        fn, ctx, check, (arr, n, lut) = self.lib.vszip_color_map, self.ctx, self.check, self._color_map_args(srcs, rs, gs, bs, lut)
        return lambda: check(fn(ctx, arr, n, lut.ctypes.data))

    def _image_unpack_args(self, srcs, planes, alphas, layout, src_bits, palette):
        n = len(srcs)
        if not (len(planes) == len(alphas) == n) or any(s.dtype != np.uint8 for s in srcs):
            raise ValueError("image_unpack: one list of planes and one alpha plane (or None) per source, sources as uint8 planes of row bytes")
        dt = planes[0][0].dtype if n else np.dtype(np.uint8)
        if any(p.dtype != dt for ps, a in zip(planes, alphas) for p in [*ps, *([a] if a is not None else [])]):
            raise ValueError("image_unpack: the planes of a call have one sample type")
        if palette is not None and not (isinstance(palette, np.ndarray) and palette.dtype == np.uint8 and palette.shape == (256, 4) and palette.flags.c_contiguous):
            raise ValueError("image_unpack: palette is a C-contiguous (256, 4) uint8 array")
        arr = (ImageUnpackFrame * n)()
        for i, (s, ps, a) in enumerate(zip(srcs, planes, alphas)):
            ps = list(ps) + [None] * (3 - len(ps))
            arr[i] = ImageUnpackFrame(s.ptr, s.stride, (C.c_void_p * 3)(*[p.ptr if p is not None else None for p in ps]), a.ptr if a is not None else None,
                                      (C.c_ssize_t * 3)(*[p.stride if p is not None else 0 for p in ps]), a.stride if a is not None else 0, ps[0].w, ps[0].h)
        return int(layout), _NP2DT[dt] if dt != np.dtype(np.uint32) else F32, int(dt.itemsize * 8 if src_bits is None else src_bits), arr, n, palette

    def image_unpack(self, srcs, planes, alphas, layout, src_bits=None, palette=None):
        """vszip.ImageRead's pixel loop on every frame: srcs the packed pixels as uint8 planes (h rows of w x pixel bytes; their stride is the
        source pitch in BYTES), planes[i] the one (grey) or three (R, G, B) output planes of frame i, alphas[i] its alpha plane or None, layout
        one of IMG_*; src_bits defaults to the sample width (1 / 2 / 4 for grey below 8 bits); palette the (256, 4) uint8 R, G, B, A table of
        IMG_INDEXED (consumed before the call returns). Float samples travel as uint32 or float32 planes. A frame's size is its first plane's."""
        layout, dt, bits, arr, n, palette = self._image_unpack_args(srcs, planes, alphas, layout, src_bits, palette)
        self.check(self.lib.vszip_image_unpack(self.ctx, layout, dt, bits, arr, n, palette.ctypes.data if palette is not None else None))

    def prepared_image_unpack(self, srcs, planes, alphas, layout, src_bits=None, palette=None):
        """-> a callable queueing vszip_image_unpack on argument blocks built once (the palette is read at every call)."""
        fn, ctx, check, (layout, dt, bits, arr, n, palette) = self.lib.vszip_image_unpack, self.ctx, self.check, self._image_unpack_args(srcs, planes, alphas, layout, src_bits, palette)
        pal = palette.ctypes.data if palette is not None else None
        return lambda: check(fn(ctx, layout, dt, bits, arr, n, pal))

    def upload_deband_tables(self, tab: dict) -> dict:
        """The tables of deband_tables() (or of the numpy spec) resident on the device, uploaded once per clip: `luma` / `chroma` as
        DevPlanes of int16 (one pair a sample), `grain_y` / `grain_c` as one-row DevPlanes or None; the host-side entries are kept."""
        dev = dict(tab)
        for k in ("luma", "chroma"):
            dev[k] = self.upload(np.ascontiguousarray(tab[k]).view(np.int16).reshape(tab[k].shape[0], tab[k].shape[1]))
        for k in ("grain_y", "grain_c"):
            dev[k] = self.upload(tab[k].reshape(1, -1)) if tab[k] is not None else None
        return dev

    def deband_entry(self, table, ssw=0, ssh=0, grain=None, grain_offset=0, grain_pitch=0, thr=0, thr1=None, thr2=None, lo=0, hi=65535) -> DebandPlane:
        """one vszip_deband_plane: `table` / `grain` are DevPlanes of upload_deband_tables (or any device memory wrapped alike)"""
        g = grain.ptr + int(grain_offset) * grain.dtype.itemsize if grain is not None else None
        return DebandPlane(table.ptr, table.stride, g, int(grain_pitch), int(ssw), int(ssh), float(thr), float(thr if thr1 is None else thr1),
                           float(thr if thr2 is None else thr2), float(lo), float(hi))

    def _deband_args(self, srcs, dsts, entries, sample_mode, blur_first, angle_boost, max_angle, max_offset):
        n = len(srcs)
        if len(entries) != n or len(dsts) != n:
            raise ValueError("deband: one destination and one vszip_deband_plane entry per plane")
        return (_NP2DT[srcs[0].dtype], self.plane_table(srcs, dsts), (DebandPlane * n)(*entries), n, int(sample_mode), int(bool(blur_first)), float(angle_boost),
                float(max_angle), int(max_offset))

    def deband(self, srcs, dsts, entries, sample_mode=2, blur_first=True, angle_boost=1.5, max_angle=0.15, max_offset=128):
        """vszip.Deband on every plane of srcs (u16 on the 16-bit scale, or f32; any sizes): entries[i] (deband_entry) names plane i's offset
        table, grain, thresholds and clamp; max_offset is the largest |value| of the tables used. dsts must not overlap srcs."""
        self.check(self.lib.vszip_deband(self.ctx, *self._deband_args(srcs, dsts, entries, sample_mode, blur_first, angle_boost, max_angle, max_offset)))

    def prepared_deband(self, srcs, dsts, entries, sample_mode=2, blur_first=True, angle_boost=1.5, max_angle=0.15, max_offset=128):
        """-> a callable queueing vszip_deband on argument blocks built once."""
        fn, ctx, check, args = self.lib.vszip_deband, self.ctx, self.check, self._deband_args(srcs, dsts, entries, sample_mode, blur_first, angle_boost, max_angle, max_offset)
        return lambda: check(fn(ctx, *args))

    def deband_lowbit(self, srcs, dsts, entries, bits, full_range=False, sample_mode=2, blur_first=True, angle_boost=1.5, max_angle=0.15, max_offset=128):
        """vszip.Deband on planes of `bits` = 8..15 (u8 for 8, else u16), resident: up to 16 bits, vszip_deband's kernels, error-diffusion dither
        back. entries as for deband(), on the 16-bit scale. full_range declares every plane non-chroma."""
        self.check(self.lib.vszip_deband_lowbit(self.ctx, *self._deband_lowbit_args(srcs, dsts, entries, bits, full_range, sample_mode, blur_first, angle_boost, max_angle,
                                                                                     max_offset)))

    def prepared_deband_lowbit(self, srcs, dsts, entries, bits, full_range=False, sample_mode=2, blur_first=True, angle_boost=1.5, max_angle=0.15, max_offset=128):
        """-> a callable queueing vszip_deband_lowbit on argument blocks built once."""
        fn, ctx, check = self.lib.vszip_deband_lowbit, self.ctx, self.check
        args = self._deband_lowbit_args(srcs, dsts, entries, bits, full_range, sample_mode, blur_first, angle_boost, max_angle, max_offset)
        return lambda: check(fn(ctx, *args))

    def _deband_lowbit_args(self, srcs, dsts, entries, bits, full_range, sample_mode, blur_first, angle_boost, max_angle, max_offset):
        want = np.uint8 if int(bits) == 8 else np.uint16
        if any(p.dtype != want for p in (*srcs, *dsts)):
            raise ValueError(f"deband_lowbit: bits={bits} takes {np.dtype(want).name} planes")
        return (int(bits), int(bool(full_range))) + self._deband_args(srcs, dsts, entries, sample_mode, blur_first, angle_boost, max_angle, max_offset)[1:]

    def _depth_args(self, srcs, dsts, bits_in, bits_out, dither, full_range, chroma):
        n = len(srcs)
        ch = [int(bool(chroma))] * n if chroma is None or np.isscalar(chroma) else [int(bool(c)) for c in chroma]
        if len(dsts) != n or len(ch) != n:
            raise ValueError("depth: one destination (and one chroma flag) per plane")
        for name, ps, bits in (("source", srcs, bits_in), ("destination", dsts, bits_out)):
            want = np.uint8 if int(bits) == 8 else np.uint16
            if 8 <= int(bits) <= 16 and any(p.dtype != want for p in ps):
                raise ValueError(f"depth: {bits}-bit {name} planes are {np.dtype(want).name}")
        if any((s.w, s.h) != (d.w, d.h) for s, d in zip(srcs, dsts)):
            raise ValueError("depth: a destination has its source's size")
        arr = (DepthPlane * n)()
        for i in range(n):
            arr[i] = DepthPlane(srcs[i].ptr, srcs[i].stride, dsts[i].ptr, dsts[i].stride, srcs[i].w, srcs[i].h, ch[i])
        return (arr, n, int(bits_in), int(bits_out), int(dither), int(bool(full_range)))

    def depth(self, srcs, dsts, bits_in, bits_out, dither=DITHER_NONE, full_range=False, chroma=None):
        """vszip_depth on every plane: srcs at bits_in, dsts at bits_out (u8 for 8 bits, u16 for 9..16), any mix of sizes; dither DITHER_NONE or
        DITHER_ERROR_DIFFUSION; chroma a scalar or one flag per plane (full-range chroma is VSZIP_ERR_UNSUPPORTED). dsts overlap no source."""
        self.check(self.lib.vszip_depth(self.ctx, *self._depth_args(srcs, dsts, bits_in, bits_out, dither, full_range, chroma)))

    def prepared_depth(self, srcs, dsts, bits_in, bits_out, dither=DITHER_NONE, full_range=False, chroma=None):
        """-> a callable queueing vszip_depth on argument blocks built once."""
        fn, ctx, check, args = self.lib.vszip_depth, self.ctx, self.check, self._depth_args(srcs, dsts, bits_in, bits_out, dither, full_range, chroma)
        return lambda: check(fn(ctx, *args))

    def _depth_fmt_args(self, srcs, dsts, dtype_in, bits_in, dtype_out, bits_out, dither, full_range, chroma):
        n = len(srcs)
        ch = [int(bool(chroma))] * n if chroma is None or np.isscalar(chroma) else [int(bool(c)) for c in chroma]
        if len(dsts) != n or len(ch) != n:
            raise ValueError("depth_fmt: one destination (and one chroma flag) per plane")
        for name, ps, dt in (("source", srcs, dtype_in), ("destination", dsts, dtype_out)):
            if int(dt) in (U8, U16, F16, F32) and any(p.dtype != _DT2NP[int(dt)] for p in ps):
                raise ValueError(f"depth_fmt: {name} planes are {_DT2NP[int(dt)].name}")
        if any((s.w, s.h) != (d.w, d.h) for s, d in zip(srcs, dsts)):
            raise ValueError("depth_fmt: a destination has its source's size")
        arr = (DepthPlane * n)()
        for i in range(n):
            arr[i] = DepthPlane(srcs[i].ptr, srcs[i].stride, dsts[i].ptr, dsts[i].stride, srcs[i].w, srcs[i].h, ch[i])
        return (arr, n, int(dtype_in), int(bits_in), int(dtype_out), int(bits_out), int(dither), int(bool(full_range)))

    def depth_fmt(self, srcs, dsts, dtype_in, bits_in, dtype_out, bits_out, dither=DITHER_NONE, full_range=False, chroma=None):
        """vszip_depth_fmt on every plane: srcs of dtype_in / bits_in, dsts of dtype_out / bits_out (U8: 8, U16: 9..16, F16: 16, F32: 32), any mix of
        sizes; full_range describes the integer side; chroma a scalar or one flag per plane. Error diffusion (DITHER_ERROR_DIFFUSION) to integers
        from float planes is served at full range, non-chroma (VSZIP_ERR_UNSUPPORTED otherwise). dsts overlap no source."""
        self.check(self.lib.vszip_depth_fmt(self.ctx, *self._depth_fmt_args(srcs, dsts, dtype_in, bits_in, dtype_out, bits_out, dither, full_range, chroma)))

    def prepared_depth_fmt(self, srcs, dsts, dtype_in, bits_in, dtype_out, bits_out, dither=DITHER_NONE, full_range=False, chroma=None):
        """-> a callable queueing vszip_depth_fmt on argument blocks built once."""
        fn, ctx, check = self.lib.vszip_depth_fmt, self.ctx, self.check
        args = self._depth_fmt_args(srcs, dsts, dtype_in, bits_in, dtype_out, bits_out, dither, full_range, chroma)
        return lambda: check(fn(ctx, *args))

    def upload_bilateral_dither_points(self, pts: np.ndarray) -> DevPlane:
        """the (23, K, 2) int16 lists of bilateral_dither_points() (or of the numpy spec) as one row of 23 * K * 2 values on the device"""
        return self.upload(np.ascontiguousarray(pts, np.int16).reshape(1, -1))

    def bilateral_dither_entry(self, radius, m, wmax, sum_w_min, points=None, K=0) -> BilateralDitherPlane:
        """one vszip_bilateral_dither_plane: m / wmax / sum_w_min / K of bilateral_dither_params(), `points` the DevPlane of
        upload_bilateral_dither_points (None: the dense window)"""
        return BilateralDitherPlane(int(radius), float(m), float(wmax), float(sum_w_min), points.ptr if points is not None else None, int(K))

    def _bilateral_dither_args(self, srcs, dsts, entries, refs, bits):
        n = len(srcs)
        if len(entries) != n or len(dsts) != n or (refs is not None and len(refs) != n):
            raise ValueError("bilateral_dither: one destination, one vszip_bilateral_dither_plane entry (and one ref or None) per plane")
        dt = srcs[0].dtype
        return (_NP2DT[dt], int(bits) if bits is not None else 8 * dt.itemsize, self.plane_table(srcs, dsts, refs), (BilateralDitherPlane * n)(*entries), n)

    def bilateral_dither(self, srcs, dsts, entries, refs=None, bits=None):
        """vszip.BilateralDither on every plane of srcs (u8, u16 with `bits` 9..16, or f32; any sizes): entries[i] (bilateral_dither_entry) names
        plane i's radius, weights and point lists; refs[i] (optional) drives the weights. dsts must overlap no input."""
        self.check(self.lib.vszip_bilateral_dither(self.ctx, *self._bilateral_dither_args(srcs, dsts, entries, refs, bits)))

    def prepared_bilateral_dither(self, srcs, dsts, entries, refs=None, bits=None):
        """-> a callable queueing vszip_bilateral_dither on argument blocks built once."""
        fn, ctx, check, args = self.lib.vszip_bilateral_dither, self.ctx, self.check, self._bilateral_dither_args(srcs, dsts, entries, refs, bits)
        return lambda: check(fn(ctx, *args))

    def prepared_limit_filter(self, flts, srcs, dsts, dark_thr, bright_thr, elast):
        """-> a callable queueing vszip_limit_filter (no third clip) on argument blocks built once."""
        n = len(flts)
        table = self.plane_table(flts, dsts, srcs)
        fa = lambda v: (C.c_float * n)(*[float(x) for x in v])
        d, b, e = fa(dark_thr), fa(bright_thr), fa(elast)
        dt, fn, ctx, check = _NP2DT[flts[0].dtype], self.lib.vszip_limit_filter, self.ctx, self.check
        return lambda: check(fn(ctx, dt, table, None, None, n, d, b, e))

    def limit_filter(self, flts, srcs, dsts, dark_thr, bright_thr, elast, refs=None):
        """vszip.LimitFilter per plane; thresholds already on the clip's scale. refs: optional third clip's planes."""
        n = len(flts)
        table = self.plane_table(flts, dsts, srcs)
        fa = lambda v: (C.c_float * n)(*[float(x) for x in v])
        rp = (C.c_void_p * n)(*[p.ptr for p in refs]) if refs is not None else None
        rs = (C.c_ssize_t * n)(*[p.stride for p in refs]) if refs is not None else None
        self.check(self.lib.vszip_limit_filter(self.ctx, _NP2DT[flts[0].dtype], table, rp, rs, n, fa(dark_thr), fa(bright_thr), fa(elast)))

    def adaptive_binarize(self, clips, clips2, dsts, c=3):
        """dsts[i] = 255 where clips2[i] - clips[i] >= c else 0 (u8 planes)."""
        self.check(self.lib.vszip_adaptive_binarize(self.ctx, self.plane_table(clips, dsts, clips2), len(clips), int(c)))

    def prepared_plane_average(self, srcs, exclude=(), refs=None, bits=None):
        """-> a callable running vszip_plane_average on argument blocks built once (a per-frame caller in C pays no Python marshalling either);
        it returns the ctypes result arrays (avg, diff)."""
        n = len(srcs)
        table = self.plane_table(srcs, None, refs)
        ex = (C.c_int32 * max(1, len(exclude)))(*exclude)
        avg, diff = (C.c_double * n)(), (C.c_double * n)()
        b = bits if bits is not None else 8 * srcs[0].dtype.itemsize
        dt, nex, fn, ctx, check = _NP2DT[srcs[0].dtype], len(exclude), self.lib.vszip_plane_average, self.ctx, self.check

        def run():
            check(fn(ctx, dt, table, n, ex, nex, b, avg, diff))
            return avg, diff
        return run

    def prepared_plane_minmax(self, srcs, minthr=0.0, maxthr=0.0, refs=None, bits=None):
        """-> a callable running vszip_plane_minmax on argument blocks built once; it returns the ctypes result arrays (min, max, diff)."""
        n = len(srcs)
        table = self.plane_table(srcs, None, refs)
        mn, mx, df = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
        b = bits if bits is not None else 8 * srcs[0].dtype.itemsize
        dt, fn, ctx, check = _NP2DT[srcs[0].dtype], self.lib.vszip_plane_minmax, self.ctx, self.check

        def run():
            check(fn(ctx, dt, table, n, minthr, maxthr, b, mn, mx, df))
            return mn, mx, df
        return run

    def plane_minmax(self, srcs, minthr=0.0, maxthr=0.0, refs=None, bits=None):
        n = len(srcs)
        table = self.plane_table(srcs, None, refs)
        mn, mx, df = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
        b = bits if bits is not None else 8 * srcs[0].dtype.itemsize
        self.check(self.lib.vszip_plane_minmax(self.ctx, _NP2DT[srcs[0].dtype], table, n, minthr, maxthr, b, mn, mx, df))
        return list(mn), list(mx), (list(df) if refs is not None else None)

    @staticmethod
    def _arr3(vals, default):
        out = []
        for i in range(3):
            out.append(vals[i] if i < len(vals) else (default if i == 0 else out[i - 1]))
        return out

    def bilateral_cfg(self, sigmaS=(), sigmaR=(), algorithm=(), pbficnum=(), planes=(True, True, True), yuv=False, ssw=0, ssh=0, hist_len=65536):
        """bilateralCreate: derive the 3 per-plane configs and build their LUTs on the device."""
        sS = (C.c_double * 3)(*(list(sigmaS) + [0.0] * 3)[:3])
        sR = (C.c_double * 3)(*self._arr3(list(sigmaR), 0.02))
        al = (C.c_int * 3)(*self._arr3(list(algorithm), 0))
        pb = (C.c_int * 3)(*self._arr3(list(pbficnum), 0))
        pl = (C.c_int * 3)(*[int(bool(x)) for x in planes])
        cfg = (BilateralCfg * 3)()
        rc = self.lib.vszip_bilateral_derive(sS, len(sigmaS), sR, al, pb, int(yuv), ssw, ssh, pl, cfg)
        if rc != OK:
            raise VszipError(rc, "Bilateral: invalid parameters")
        for i in range(3):
            self.check(self.lib.vszip_bilateral_luts(self.ctx, C.byref(cfg[i]), hist_len))
        return cfg

    def bilateral_free(self, cfg):
        for i in range(3):
            for f in ("gs_lut", "gr_lut"):
                p = getattr(cfg[i], f)
                if p:
                    self.lib.vszip_dev_free(self.ctx, p)
                    setattr(cfg[i], f, None)

    def bilateral(self, srcs, dsts, cfg, plane_index, refs=None, peak=None):
        """plane_index[i] = which of the 3 configs plane i uses."""
        n = len(srcs)
        table = self.plane_table(srcs, dsts, refs)
        ptrs = (C.POINTER(BilateralCfg) * n)(*[C.pointer(cfg[k]) for k in plane_index])
        dt = srcs[0].dtype
        if peak is None:
            peak = float((1 << (8 * dt.itemsize)) - 1) if dt.kind == "u" else 65535.0
        self.check(self.lib.vszip_bilateral(self.ctx, _NP2DT[dt], table, ptrs, n, peak))

    def ssimulacra2(self, ref_planes, dis_planes):
        """ref_planes / dis_planes: flat lists of 3*npairs f32 DevPlanes (same geometry). -> scores[npairs]"""
        n = len(ref_planes) // 3
        r = (C.c_void_p * (3 * n))(*[p.ptr for p in ref_planes])
        d = (C.c_void_p * (3 * n))(*[p.ptr for p in dis_planes])
        out = (C.c_double * n)()
        p0 = ref_planes[0]
        self.check(self.lib.vszip_ssimulacra2(self.ctx, r, d, p0.stride, p0.w, p0.h, n, out))
        return list(out)

    def chain_run(self, stages, srcs, dsts, plane_slot):
        """stages: list of dicts — {"boxblur": (hr, hp, vr, vp)} | {"bilateral": cfg, "peak": p} | {"limiter": (lo3, hi3)}, each with
        an optional "planes": (bool, bool, bool). One call: every stage on the resident planes, intermediates owned by the context."""
        arr = (ChainStage * len(stages))()
        for st, d in zip(arr, stages):
            pr = d.get("planes", (True, True, True))
            for k in range(3):
                st.process[k] = int(bool(pr[k]))
            if "boxblur" in d:
                st.kind = STAGE_BOXBLUR
                st.hradius, st.hpasses, st.vradius, st.vpasses = d["boxblur"]
            elif "bilateral" in d:
                st.kind = STAGE_BILATERAL
                for k in range(3):
                    st.bilateral[k] = C.pointer(d["bilateral"][k])
                    st.process[k] = int(bool(pr[k]) and bool(d["bilateral"][k].process))
                st.peak = d["peak"]
            else:
                st.kind = STAGE_LIMITER
                for k in range(3):
                    st.lo[k], st.hi[k] = d["limiter"][0][k], d["limiter"][1][k]
        n = len(srcs)
        slots = (C.c_int * n)(*plane_slot)
        self.check(self.lib.vszip_chain_run(self.ctx, _NP2DT[srcs[0].dtype], arr, len(stages), self.plane_table(srcs, dsts), slots, n))

    def chain_ops(self, ops, srcs, dsts, plane_slot, frames=None, bits=None):
        """vszip_chain_ops: a chain over every frame-in / frame-out filter on resident planes in one call, intermediates owned by the context.
        ops: list of dicts, one key per kind and an optional "planes": (bool, bool, bool) each -
          {"boxblur": (hr, hp, vr, vp)} | {"bilateral": cfg, "peak": p} | {"limiter": (lo3, hi3)}                       as chain_run
          {"clahe": (limit, tiles)} | {"comb_mask": dict(cthresh, mthresh, expand, metric)} | {"comb_mask_mt": (thY1, thY2)}
          {"checkmate": dict(thr, tmax, tthr2)} | {"compress": tables, "chroma": per entry | scalar | None}
          {"mosquito_nr": dict(strength, restore, radius, chroma)}      scalars, or one value per table ENTRY (len(srcs) values)
          {"deband": entries, sample_mode=, blur_first=, angle_boost=, max_angle=, max_offset=}   entries: one deband_entry per table entry (None
                                                                                                  where the op skips the entry)
          {"bilateral_dither": entries}                                 one bilateral_dither_entry per table entry (None where skipped)
        plane_slot[i] in 0..2; frames[i]: the frame number of entry i (needed by checkmate and by comb_mask with mthresh > 0: the table is a
        clip, and the neighbouring frames are the table's other entries of the slot, as the op before left them). bits: bits per sample for
        mosquito_nr / bilateral_dither (default: the sample width)."""
        args, _keep = self._chain_ops_args(ops, srcs, dsts, plane_slot, frames, bits)
        self.check(self.lib.vszip_chain_ops(self.ctx, *args))

    def _chain_ops_args(self, ops, srcs, dsts, plane_slot, frames=None, bits=None):
        """the argument blocks of vszip_chain_ops for chain_ops() / prepared_chain_ops(), and what must stay alive while they are used"""
        n = len(srcs)
        keep = []  # the params blocks: alive until the call returns

        def hold(x):
            keep.append(x)
            return x

        def per_entry(v, ctype, default=None):
            if v is None:
                v = default
            if v is None:
                return None
            vals = [v] * n if isinstance(v, (bool, int, np.integer)) else list(v)
            if len(vals) != n:
                raise ValueError("chain_ops: a per-plane parameter is a scalar or has one value per table entry")
            return hold((ctype * n)(*[int(x) for x in vals]))

        def structs(entries, cls):
            if len(entries) != n:
                raise ValueError("chain_ops: one parameter entry (or None) per table entry")
            return hold((cls * n)(*[e if e is not None else cls() for e in entries]))

        arr = (ChainOp * len(ops))()
        for op, d in zip(arr, ops):
            pr = d.get("planes", (True, True, True))
            for k in range(3):
                op.process[k] = int(bool(pr[k]))
            if "boxblur" in d:
                op.kind, prm = STAGE_BOXBLUR, ChainBoxBlur(*[int(v) for v in d["boxblur"]])
            elif "bilateral" in d:
                op.kind, prm = STAGE_BILATERAL, ChainBilateral()
                for k in range(3):
                    prm.cfg[k] = C.pointer(d["bilateral"][k])
                    op.process[k] = int(bool(pr[k]) and bool(d["bilateral"][k].process))
                prm.peak = d["peak"]
            elif "limiter" in d:
                op.kind, prm = STAGE_LIMITER, ChainLimiter()
                for k in range(3):
                    prm.lo[k], prm.hi[k] = d["limiter"][0][k], d["limiter"][1][k]
            elif "clahe" in d:
                limit, tiles = d["clahe"]
                op.kind, prm = STAGE_CLAHE, ChainClahe(int(limit), *self.clahe_tiles(tiles))
            elif "comb_mask" in d:
                a = dict(cthresh=6, mthresh=9, expand=True, metric=0)
                a.update(d["comb_mask"])
                op.kind, prm = STAGE_COMB_MASK, ChainCombMask(int(a["cthresh"]), int(a["mthresh"]), int(bool(a["expand"])), int(a["metric"]))
            elif "comb_mask_mt" in d:
                op.kind, prm = STAGE_COMB_MASK_MT, ChainCombMaskMT(*[int(v) for v in d["comb_mask_mt"]])
            elif "checkmate" in d:
                a = dict(thr=12, tmax=12, tthr2=0)
                a.update(d["checkmate"])
                op.kind, prm = STAGE_CHECKMATE, ChainCheckmate(int(a["thr"]), int(a["tmax"]), int(a["tthr2"]))
            elif "mosquito_nr" in d:
                a = d["mosquito_nr"]
                op.kind, prm = STAGE_MOSQUITO_NR, ChainMosquitoNR(per_entry(a.get("strength"), C.c_int32, 16), per_entry(a.get("restore"), C.c_int32, 128),
                                                                  per_entry(a.get("radius"), C.c_int32, 2), per_entry(a.get("chroma"), C.c_uint8))
            elif "deband" in d:
                op.kind, prm = STAGE_DEBAND, ChainDeband(structs(d["deband"], DebandPlane), int(d.get("sample_mode", 2)), int(bool(d.get("blur_first", True))),
                                                         float(d.get("angle_boost", 1.5)), float(d.get("max_angle", 0.15)), int(d.get("max_offset", 128)))
            elif "bilateral_dither" in d:
                op.kind, prm = STAGE_BILATERAL_DITHER, ChainBilateralDither(structs(d["bilateral_dither"], BilateralDitherPlane))
            elif "compress" in d:
                op.kind, prm = STAGE_COMPRESS, ChainCompress(C.pointer(d["compress"]) if d["compress"] is not None else None, per_entry(d.get("chroma"), C.c_uint8))
            elif "raw" in d:  # (kind, address of a params block or None): what a C host could pass (tests of the refusals)
                op.kind, prm = int(d["raw"][0]), None
                op.params = d["raw"][1]
            else:
                raise ValueError(f"chain_ops: no known kind in {sorted(d)}")
            if prm is not None:
                op.params = C.addressof(hold(prm))
        dt = srcs[0].dtype
        slots = (C.c_int * n)(*plane_slot)
        fr = (C.c_int * n)(*[int(f) for f in frames]) if frames is not None else None
        b = int(bits) if bits is not None else 8 * dt.itemsize
        return (_NP2DT[dt], b, arr, len(ops), self.plane_table(srcs, dsts), slots, fr, n), keep

    def prepared_chain_ops(self, ops, srcs, dsts, plane_slot, frames=None, bits=None):
        """-> a callable queueing vszip_chain_ops on argument blocks built once."""
        fn, ctx, check, (args, keep) = self.lib.vszip_chain_ops, self.ctx, self.check, self._chain_ops_args(ops, srcs, dsts, plane_slot, frames, bits)
        return lambda _keep=keep: check(fn(ctx, *args))

    @staticmethod
    def ssim_source(family: str, dtype, bits=None, linearize=True, limited=None, ssw=0, ssh=0, matrix=1, chroma_loc=0) -> SsimSource:
        """family "RGB" | "GRAY" | "YUV"; integer samples: full range for RGB, limited for Gray / YUV (zimg's defaults) unless
        given. YUV: log2 subsampling, _Matrix, _ChromaLocation (the chroma row pitch is filled in from the planes)."""
        dt = np.dtype(dtype)
        fam = {"GRAY": CF_GRAY, "YUV": CF_YUV}.get(family.upper(), CF_RGB)
        b = bits if bits is not None else (32 if dt.kind == "f" else 8 * dt.itemsize)
        lim = (fam != CF_RGB) if limited is None else bool(limited)
        return SsimSource(fam, _NP2DT[dt], b, int(lim and dt.kind != "f"), int(bool(linearize)), ssw, ssh, matrix, chroma_loc, 0)

    def ssimulacra2_src(self, fmt: SsimSource, ref_planes, dis_planes):
        """SSIMULACRA2 with the colour pre-stage on the device: ref_planes / dis_planes are flat lists of
        npairs * (3 | 1) source DevPlanes in the clip's own sample type. -> scores[npairs]"""
        per = 1 if fmt.family == CF_GRAY else 3
        n = len(ref_planes) // per
        r = (C.c_void_p * (per * n))(*[p.ptr for p in ref_planes])
        d = (C.c_void_p * (per * n))(*[p.ptr for p in dis_planes])
        out = (C.c_double * n)()
        p0 = ref_planes[0]
        if fmt.family == CF_YUV:
            fmt.chroma_stride = ref_planes[1].stride
            assert all(p.stride == (p0.stride if i % 3 == 0 else fmt.chroma_stride) for i, p in enumerate(list(ref_planes) + list(dis_planes)))
        self.check(self.lib.vszip_ssimulacra2_src(self.ctx, C.byref(fmt), r, d, p0.stride, p0.w, p0.h, n, out))
        return list(out)

    def to_rgbs_linear(self, fmt: SsimSource, planes):
        """One frame's source planes -> [R, G, B] linear-light f32 DevPlanes (hz.toRGBS + sRGBtoLinearRGB)."""
        p0 = planes[0]
        dst = [self.empty(p0.h, p0.w, np.float32) for _ in range(3)]
        self.to_rgbs_linear_into(fmt, planes, dst)
        self.sync()
        return dst

    def to_rgbs_linear_into(self, fmt: SsimSource, planes, dst):
        """to_rgbs_linear() into three f32 planes the caller brings (one pitch); asynchronous"""
        p0 = planes[0]
        per = 1 if fmt.family == CF_GRAY else 3
        s = (C.c_void_p * per)(*[p.ptr for p in planes[:per]])
        d = (C.c_void_p * 3)(*[p.ptr for p in dst])
        assert dst[0].stride == dst[1].stride == dst[2].stride
        if fmt.family == CF_YUV:
            fmt.chroma_stride = planes[1].stride
        self.check(self.lib.vszip_to_rgbs_linear(self.ctx, C.byref(fmt), s, p0.stride, d, dst[0].stride, p0.w, p0.h))

    def eedi3(self, srcs, field, dh=False, alpha=0.2, beta=0.25, gamma=20.0, nrad=2, mdis=20, hp=False, vcheck=2,
              vthresh0=32.0, vthresh1=64.0, vthresh2=4.0, sclips=None, horizontal=False, mclips=None):
        """srcs: f32 DevPlanes; mclips: optional u8 DevPlanes with the geometry of srcs. Returns the output DevPlanes."""
        dsts = []
        for s in srcs:
            if horizontal:
                dsts.append(self.empty(s.h, s.w * 2 if dh else s.w, np.float32))
            else:
                dsts.append(self.empty(s.h * 2 if dh else s.h, s.w, np.float32))
        self.eedi3_into(srcs, dsts, field, dh, alpha, beta, gamma, nrad, mdis, hp, vcheck, vthresh0, vthresh1, vthresh2, sclips, horizontal, mclips)
        return dsts

    def eedi3_into(self, srcs, dsts, field, dh=False, alpha=0.2, beta=0.25, gamma=20.0, nrad=2, mdis=20, hp=False, vcheck=2,
                   vthresh0=32.0, vthresh1=64.0, vthresh2=4.0, sclips=None, horizontal=False, mclips=None):
        """eedi3() on output planes the caller brings (dsts[i]: the geometry vszip_eedi3 states for planes[i].dst)."""
        n = len(srcs)
        table = self.plane_table(srcs, dsts)
        prm = Eedi3Params(int(dh), alpha, beta, gamma, nrad, mdis, int(hp), vcheck, vthresh0, vthresh1, vthresh2)
        if sclips is not None:
            sp = (C.c_void_p * n)(*[(s.ptr if s is not None else None) for s in sclips])
            ss = (C.c_ssize_t * n)(*[(s.stride if s is not None else 0) for s in sclips])
        else:
            sp, ss = None, None
        if mclips is not None:
            mp = (C.c_void_p * n)(*[(m.ptr if m is not None else None) for m in mclips])
            ms = (C.c_ssize_t * n)(*[(m.stride if m is not None else 0) for m in mclips])
            self.check(self.lib.vszip_eedi3_mclip(self.ctx, table, sp, ss, mp, ms, n, field, int(horizontal), C.byref(prm)))
        else:
            self.check(self.lib.vszip_eedi3(self.ctx, table, sp, ss, n, field, int(horizontal), C.byref(prm)))

    def xpsnr_wsse(self, org, rec, prev1=None, prev2=None, depth=8, frame_rate=24, temporal=True):
        """org / rec: lists of 1 or 3 DevPlanes (u8/u16). -> [wsse64 per plane]"""
        n = len(org)
        vp3 = lambda l: (C.c_void_p * 3)(*([p.ptr for p in l] + [None] * (3 - n)))
        w = (C.c_int * 3)(*([p.w for p in org] + [0] * (3 - n)))
        h = (C.c_int * 3)(*([p.h for p in org] + [0] * (3 - n)))
        st = (C.c_ssize_t * 3)(*([p.stride for p in org] + [0] * (3 - n)))
        out = (C.c_uint64 * 3)()
        self.check(self.lib.vszip_xpsnr_wsse(self.ctx, org[0].dtype.itemsize, vp3(org), vp3(rec), prev1.ptr if prev1 else None, prev2.ptr if prev2 else None,
                                             w, h, st, depth, n, frame_rate, int(temporal), out))
        return [int(out[i]) for i in range(n)]

    def xpsnr_batch_call(self, orgs, recs, prev1s=None, prev2s=None, depth=8, frame_rate=24, temporal=True):
        """The argument marshalling of xpsnr_wsse_batch done once: returns run() -> [[wsse64 per plane] per
        frame] (a host that keeps its frame pointers in C arrays pays none of it per call)."""
        nf, n = len(orgs), len(orgs[0])
        flat = lambda ll: (C.c_void_p * (nf * n))(*[p.ptr for l in ll for p in l])
        prev = lambda l: (C.c_void_p * nf)(*[(p.ptr if p is not None else None) for p in l]) if l is not None else None
        o0 = orgs[0]
        w = (C.c_int * 3)(*([p.w for p in o0] + [0] * (3 - n)))
        h = (C.c_int * 3)(*([p.h for p in o0] + [0] * (3 - n)))
        st = (C.c_ssize_t * 3)(*([p.stride for p in o0] + [0] * (3 - n)))
        out = (C.c_uint64 * (3 * nf))()
        fo, fr, p1, p2 = flat(orgs), flat(recs), prev(prev1s), prev(prev2s)
        bps, keep = o0[0].dtype.itemsize, (orgs, recs, prev1s, prev2s)

        def run(_keep=keep):
            self.check(self.lib.vszip_xpsnr_wsse_batch(self.ctx, bps, nf, fo, fr, p1, p2, w, h, st, depth, n, frame_rate, int(temporal), out))
            return [[int(out[3 * f + i]) for i in range(n)] for f in range(nf)]

        return run

    def xpsnr_wsse_batch(self, orgs, recs, prev1s=None, prev2s=None, depth=8, frame_rate=24, temporal=True):
        """orgs / recs: one list of 1 or 3 DevPlanes per frame (same geometry); prev1s / prev2s: per
        frame the luma DevPlane of frames n-1 / n-2 or None. -> [[wsse64 per plane] per frame]"""
        return self.xpsnr_batch_call(orgs, recs, prev1s, prev2s, depth, frame_rate, temporal)()
