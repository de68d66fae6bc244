"""The parity spec of vszip_depth and vszip_deband_lowbit in numpy: integer depth conversion as zimg's scalar path does it
(resize.Point with dither_type none / error_diffusion, which is what hz.bitDepth of the reference's src/helper.zig:470-494 asks
for around Deband and XPSNR), and Deband on clips under 16 bits as src/vapoursynth/deband.zig:462-497 wraps it.

Arithmetic: IEEE f32, every product and every sum rounded on its own, in the order written here.
  scale   limited range 2^(bits_out - bits_in); full range, non-chroma (2^bits_out - 1) / (2^bits_in - 1) divided in f64, rounded to f32
  none    q = rint(min(max(src * scale, 0), peak)), half to even
  error diffusion (Floyd-Steinberg, rows top to bottom, samples left to right; errors outside the plane are 0):
          err = 0 + left * 7/16;  err += top[x + 1] * 3/16;  err += top[x] * 5/16;  err += top[x - 1] * 1/16
          v = min(max(src * scale + err, 0), peak);  q = rint(v);  the sample's error is v - q
Full-range chroma has an offset whose rounding no recorded data pins: not served (VSZIP_ERR_UNSUPPORTED). The three 8-bit goldens of
Deband (deband_ref.LEFT_OUT) pin the limited-range error diffusion 16 -> 8 exactly; the full-range non-chroma case rests on this
restatement alone.

Two builders of the error diffusion: a serial one (the recurrence as written) and a fast one, vectorised along the anti-diagonals
t = x + 2 y (all samples of one t depend on earlier t only); tests/test_depth_ref.py shows they agree."""
from __future__ import annotations

import numpy as np

import deband_ref as db

F = np.float32
NONE, ERROR_DIFFUSION = 0, 1
ERR_ARG, ERR_UNSUPPORTED = -1, -3
K_LEFT, K_TOP_P1, K_TOP_0, K_TOP_M1 = F(7.0) / F(16.0), F(3.0) / F(16.0), F(5.0) / F(16.0), F(1.0) / F(16.0)


class DepthError(ValueError):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


def dtype_of(bits: int):
    return np.uint8 if bits == 8 else np.uint16


def check_args(bits_in, bits_out, dither, full_range, planes) -> None:
    """the checks of vszip_depth in its order, with its texts; planes: (has_src, has_dst, w, h, src_stride, dst_stride, chroma) each"""
    if not 8 <= bits_in <= 16:
        raise DepthError(ERR_ARG, f"Depth: bits_in {bits_in} is outside 8..16")
    if not 8 <= bits_out <= 16:
        raise DepthError(ERR_ARG, f"Depth: bits_out {bits_out} is outside 8..16")
    if dither not in (NONE, ERROR_DIFFUSION):
        raise DepthError(ERR_ARG, f"Depth: dither {dither} is neither 0 (none) nor 1 (error diffusion)")
    if not planes:
        raise DepthError(ERR_ARG, "Depth: no planes")
    for i, (has_src, has_dst, w, h, ss, ds, chroma) in enumerate(planes):
        if not has_src or not has_dst:
            raise DepthError(ERR_ARG, f"Depth: plane {i}: src and dst must not be NULL")
        if w < 1 or h < 1 or ss < w or ds < w or max(ss, ds) > 2**31 - 1:
            raise DepthError(ERR_ARG, f"Depth: plane {i}: bad geometry {w}x{h}, pitches {ss} -> {ds}")
        if full_range and chroma:
            raise DepthError(ERR_UNSUPPORTED, f"Depth: plane {i}: full-range chroma is not built (DESIGN.md section 1)")


def scale_of(bits_in: int, bits_out: int, full_range: bool = False) -> np.float32:
    if not full_range:
        return F(2.0 ** (bits_out - bits_in))  # exact
    return F(float(2**bits_out - 1) / float(2**bits_in - 1))


def _none(src, scale, peak):
    return np.rint(np.minimum(np.maximum(src.astype(F) * scale, F(0)), peak))


def _diffuse_serial(src, scale, peak):
    h, w = src.shape
    out = np.empty((h, w), F)
    top = np.zeros(w + 2, F)  # top[x + 1]: the error of the row above at x
    for y in range(h):
        cur = np.zeros(w + 2, F)
        left = F(0)
        for x in range(w):
            x0 = F(src[y, x]) * scale
            err = F(0) + left * K_LEFT
            err = err + top[x + 2] * K_TOP_P1
            err = err + top[x + 1] * K_TOP_0
            err = err + top[x] * K_TOP_M1
            v = min(max(x0 + err, F(0)), peak)
            q = np.rint(v)
            out[y, x] = q
            left = cur[x + 1] = v - q
        top = cur
    return out


def _diffuse_fast(src, scale, peak):
    h, w = src.shape
    out = np.empty((h, w), F)
    x0 = src.astype(F) * scale
    e = np.zeros((h + 1, w + 2), F)  # e[y + 1, x + 1]: the error of sample (y, x); row 0 and the outer columns stay 0
    for t in range(w + 2 * (h - 1)):
        ys = np.arange(max(0, (t - w + 2) // 2), min(h - 1, t // 2) + 1)
        xs = t - 2 * ys
        err = F(0) + e[ys + 1, xs] * K_LEFT
        err = err + e[ys, xs + 2] * K_TOP_P1
        err = err + e[ys, xs + 1] * K_TOP_0
        err = err + e[ys, xs] * K_TOP_M1
        v = np.minimum(np.maximum(x0[ys, xs] + err, F(0)), peak)
        q = np.rint(v)
        out[ys, xs] = q
        e[ys + 1, xs + 1] = v - q
    return out


def convert(src: np.ndarray, bits_in: int, bits_out: int, dither: int = NONE, full_range: bool = False, chroma: bool = False, fast: bool = True) -> np.ndarray:
    """one plane at bits_in (uint8 for 8, uint16 above) -> the plane at bits_out"""
    h, w = src.shape
    check_args(bits_in, bits_out, dither, full_range, [(True, True, w, h, w, w, chroma)])
    assert src.dtype == dtype_of(bits_in), (src.dtype, bits_in)
    scale, peak = scale_of(bits_in, bits_out, full_range), F(2**bits_out - 1)
    q = _none(src, scale, peak) if dither == NONE else (_diffuse_fast if fast else _diffuse_serial)(src, scale, peak)
    return q.astype(dtype_of(bits_out))


def content(seed: int, h: int, w: int, bits: int) -> np.ndarray:
    """test content at `bits`: noise with runs of five samples that hold at 0 and at the peak, so that the clamp feeds the error"""
    import fixtures as fx

    a = (fx.splitmix64_plane(seed, (h, w), np.uint16) >> np.uint16(16 - bits)).astype(np.uint16)
    r = fx.splitmix64_plane(seed + 99, (h, (w + 4) // 5), np.uint16).repeat(5, axis=1)[:, :w] % 7
    a[r == 0] = 0
    a[r == 1] = (1 << bits) - 1
    return a.astype(dtype_of(bits))


def deband_lowbit_frame(planes, bits: int, family="GRAY", ssw=0, ssh=0, full_range: bool = False, fast: bool = True, **kw) -> list:
    """vszip.Deband on a frame under 16 bits: up with dither none, deband_ref.deband_frame at 16 bits, down with error diffusion.
    The keyword arguments are deband_frame's (thresholds and grain on the wrapper's 8-bit scale, as everywhere)."""
    up = [convert(p, bits, 16, NONE, full_range, fast=fast) for p in planes]
    mid = db.deband_frame(up, family, ssw, ssh, **kw)
    return [convert(p, 16, bits, ERROR_DIFFUSION, full_range, fast=fast) for p in mid]


_FMT8 = {"GRAY8": ("GRAY", 0, 0), "YUV420P8": ("YUV", 1, 1), "YUV422P8": ("YUV", 1, 0)}


def golden_inputs8(fmt: str) -> list:
    """the inputs of the three 8-bit golden keys, from tests/fixtures.py"""
    import fixtures as fx

    family, ssw, ssh = _FMT8[fmt]
    p = [fx.crop_gray8()] if family == "GRAY" else list(fx.yuv_geometry(fx.crop_yuv(8, ssw, ssh), "full", ssw, ssh))
    return [np.ascontiguousarray(x) for x in p]


def run_key8(key: str) -> list:
    """one of deband_ref.LEFT_OUT's keys through the spec"""
    fmt, geometry, kw = db.parse_key(key)
    assert geometry == "full"
    family, ssw, ssh = _FMT8[fmt]
    return deband_lowbit_frame(golden_inputs8(fmt), 8, family, ssw, ssh, **kw)


def same_as_golden(key: str, outs) -> list:
    """the criterion the 8-bit goldens allow: min and max equal, and |avg - golden| * w * h * peak < 0.5 (the sum of all samples is
    equal). -> the planes that miss, as (plane, stats, golden)"""
    import fixtures as fx

    want, bad = db.goldens()[key], []
    for i, o in enumerate(outs):
        st, g = fx.plane_stats(o), want[f"p{i}"]
        if st["min"] != g["min"] or st["max"] != g["max"] or not abs(st["avg"] - g["avg"]) * o.size * 255 < 0.5:
            bad.append((i, st, g))
    return bad
