"""The parity spec of vszip_depth_fmt in numpy: the change of sample type between integer (8, 9..16 bits), half and float planes as zimg's
resize.Point(format=...) makes it. tests/test_depth_fmt_ref.py ties it bit for bit to oracle/vs_host.py int_to_float / float_to_int (the
steps the reference's float and YUV goldens pass through) and, for integer -> integer, to tests/depth_ref.py.

Arithmetic: IEEE f32. With off / rng of the integer side
  limited range   off = (chroma ? 128 : 16) << (bits - 8),  rng = (chroma ? 224 : 219) << (bits - 8)
  full range      off = chroma ? 2^(bits - 1) : 0,          rng = 2^bits - 1
  int -> f32               fma(v, f32(1 / rng), f32(-off / rng)), one fused operation, the constants divided in f64 and rounded once
  f32 -> int, none         q = rint(fma(x, rng, off)), half to even, clamped to [0, 2^bits - 1]; +-Inf clamp, NaN outside the contract
  f32 -> int, diffusion    off == 0 only (full range, non-chroma): depth_ref's recurrence on the float sample with scale = f32(rng)
  f16 -> f32 exact; f32 -> f16 nearest even, subnormals kept
  int <-> f16              through f32: the f32 result rounded to f16; the f16 sample widened first
Pinned by recorded data: int -> f32 and f32 -> int `none` at limited range (luma and chroma) and int -> f32 at full range non-chroma. On
this restatement alone: half planes, full-range chroma, and the error diffusion from float."""
from __future__ import annotations

import numpy as np

import depth_ref as dr
from oracle.vs_host import fma32

F = np.float32
U8, U16, F16, F32 = 0, 1, 2, 3
NONE, ERROR_DIFFUSION = 0, 1
ERR_ARG, ERR_UNSUPPORTED = -1, -3
NP = {U8: np.dtype(np.uint8), U16: np.dtype(np.uint16), F16: np.dtype(np.float16), F32: np.dtype(np.float32)}
NAME = {U8: "VSZIP_U8", U16: "VSZIP_U16", F16: "VSZIP_F16", F32: "VSZIP_F32"}
BITS = {U8: (8, 8), U16: (9, 16), F16: (16, 16), F32: (32, 32)}


def is_float(dtype: int) -> bool:
    return dtype in (F16, F32)


def dtype_for_bits(bits: int) -> int:
    return U8 if bits == 8 else U16


def range_of(bits: int, full_range: bool, chroma: bool):
    if not full_range:
        return (128 if chroma else 16) << (bits - 8), (224 if chroma else 219) << (bits - 8)
    return (1 << (bits - 1)) if chroma else 0, (1 << bits) - 1


def check_args(dtype_in, bits_in, dtype_out, bits_out, dither, full_range, planes) -> None:
    """the checks of vszip_depth_fmt in its order, with its texts; planes: (has_src, has_dst, w, h, src_stride, dst_stride, chroma) each"""
    sides = (("in", dtype_in, bits_in), ("out", dtype_out, bits_out))
    for name, dt, _ in sides:
        if dt not in NP:
            raise dr.DepthError(ERR_ARG, f"DepthFmt: dtype_{name} {dt} is none of VSZIP_U8, VSZIP_U16, VSZIP_F16, VSZIP_F32")
    for name, dt, bits in sides:
        lo, hi = BITS[dt]
        if not lo <= bits <= hi:
            raise dr.DepthError(ERR_ARG, f"DepthFmt: bits_{name} {bits} does not fit {NAME[dt]} ({lo})" if lo == hi else f"DepthFmt: bits_{name} {bits} does not fit {NAME[dt]} ({lo}..{hi})")
    if not is_float(dtype_in) and not is_float(dtype_out):
        return dr.check_args(bits_in, bits_out, dither, full_range, planes)
    if dither not in (NONE, ERROR_DIFFUSION):
        raise dr.DepthError(ERR_ARG, f"DepthFmt: dither {dither} is neither 0 (none) nor 1 (error diffusion)")
    if dither and is_float(dtype_out):
        raise dr.DepthError(ERR_ARG, f"DepthFmt: error diffusion needs an integer destination, dtype_out is {NAME[dtype_out]}")
    if not planes:
        raise dr.DepthError(ERR_ARG, "DepthFmt: no planes")
    for i, (has_src, has_dst, w, h, ss, ds, chroma) in enumerate(planes):
        if not has_src or not has_dst:
            raise dr.DepthError(ERR_ARG, f"DepthFmt: plane {i}: src and dst must not be NULL")
        if w < 1 or h < 1 or ss < w or ds < w or max(ss, ds) > 2**31 - 1:
            raise dr.DepthError(ERR_ARG, f"DepthFmt: plane {i}: bad geometry {w}x{h}, pitches {ss} -> {ds}")
        if dither and range_of(bits_out, full_range, chroma)[0] != 0:
            raise dr.DepthError(ERR_UNSUPPORTED, f"DepthFmt: plane {i}: error diffusion from float with an offset ({'chroma' if full_range else 'limited range'}) is not built (DESIGN.md section 1)")
    rows = sum(p[3] for p in planes)
    if rows > (2**31 - 1) // 2:
        raise dr.DepthError(ERR_UNSUPPORTED, f"DepthFmt: {rows} rows are more than one call numbers")


def int_to_float(plane: np.ndarray, bits: int, full_range: bool, chroma: bool = False) -> np.ndarray:
    off, rng = range_of(bits, full_range, chroma)
    return fma32(plane.astype(F), F(1.0 / rng), F(-float(off) / rng))


def float_to_int(x: np.ndarray, bits: int, full_range: bool, chroma: bool = False) -> np.ndarray:
    off, rng = range_of(bits, full_range, chroma)
    x = np.asarray(x, F)
    fin = np.isfinite(x)
    y = np.where(fin, fma32(np.where(fin, x, F(0)), F(rng), F(off)), x)  # +-Inf stay themselves and clamp
    return np.clip(np.rint(y), 0, (1 << bits) - 1).astype(dr.dtype_of(bits))


def convert(src: np.ndarray, dtype_in: int, bits_in: int, dtype_out: int, bits_out: int, dither: int = NONE, full_range: bool = False, chroma: bool = False) -> np.ndarray:
    """one plane of dtype_in / bits_in -> the plane of dtype_out / bits_out"""
    h, w = src.shape
    check_args(dtype_in, bits_in, dtype_out, bits_out, dither, full_range, [(True, True, w, h, w, w, chroma)])
    assert src.dtype == NP[dtype_in], (src.dtype, dtype_in)
    if not is_float(dtype_in) and not is_float(dtype_out):
        return dr.convert(src, bits_in, bits_out, dither, full_range, chroma)
    if not is_float(dtype_in):
        return int_to_float(src, bits_in, full_range, chroma).astype(NP[dtype_out])
    x = src.astype(F)  # f16 -> f32 is exact
    if is_float(dtype_out):
        with np.errstate(over="ignore"):
            return x.astype(NP[dtype_out])
    if dither == NONE:
        return float_to_int(x, bits_out, full_range, chroma)
    rng = range_of(bits_out, full_range, chroma)[1]
    with np.errstate(invalid="ignore"):
        return dr._diffuse_fast(x, F(rng), F(2**bits_out - 1)).astype(NP[dtype_out])


SPECIALS = (np.inf, -np.inf, -0.0, 0.0, 2.0**-24, 3 * 2.0**-24, 2.0**-14 - 2.0**-24, -(2.0**-15), 1.0, 2.0**-14)  # Inf, zeros, half subnormals


def content(seed: int, h: int, w: int, bits: int = 8, full_range: bool = True, chroma: bool = False, half: bool = False) -> np.ndarray:
    """float test content for a conversion whose integer side is (bits, full_range, chroma): noise over [-0.1, 1.1] ([-0.6, 0.6] for chroma), runs
    of five samples that hold below the range and above it (the clamp feeds the error), runs of values placed on q + 0.5 (ties), and +-Inf, +-0
    and half subnormals scattered over the plane. No NaN."""
    import fixtures as fx

    lo, hi = (-0.6, 0.6) if chroma else (-0.1, 1.1)
    u = fx.splitmix64_plane(seed, (h, w), np.uint16).astype(np.float64) / 65535.0
    a = (lo + (hi - lo) * u).astype(F)
    r = fx.splitmix64_plane(seed + 99, (h, (w + 4) // 5), np.uint16).repeat(5, axis=1)[:, :w] % 9
    a[r == 0] = F(lo - 0.05)  # beyond either clamp at limited range too
    a[r == 1] = F(hi + 0.05)
    off, rng = range_of(bits, full_range, chroma)
    q = (fx.splitmix64_plane(seed + 7, (h, w), np.uint16) % np.uint16(min(1 << bits, 1 << 15))).astype(np.float64)
    a = np.where(r == 2, ((q + 0.5 - off) / rng).astype(F), a)
    flat = a.reshape(-1)
    for k, v in enumerate(SPECIALS):
        flat[(5 + 11 * k) % flat.size] = F(v)
    a = flat.reshape(h, w)
    return a.astype(np.float16) if half else a
