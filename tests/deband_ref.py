"""Parity spec of vszip.Deband (f3kdb-style debanding with grain) in numpy: what src/vapoursynth/deband.zig builds at
create time (seed mix, the three random generators, the offset tables, the grain buffers, the per-frame grain offsets)
and what processPlane of src/filters/deband_int.zig / deband_float.zig computes per sample, in all seven sample modes,
for 16-bit integer and 32-bit float planes, plus the wrapper's per-plane mapping of thr / grain / clamps.

Formulation. The reference stores FLAT offsets (val * stride, or stride * val2 + val1) and reads src[base +- flat]. The
tables here hold the raw refEncode()d pairs (val1, val2) and the filter reads src[y +- dy][x +- dx]: every reference sample
lies inside the plane (cur_range never exceeds the distance to the nearest edge; the signed-char quirk abs(-128) == -128
needs cur_range >= 128 and is in range both ways), so both address the same sample and no clamp takes part.

The reference's output depends on VapourSynth's row pitch through the grain index grain[y * stride + x]; the goldens
were made with 32-byte frame alignment (`align`), and the grain pitch is an argument everywhere below.

Float pairing. The float path takes @abs() of the flattened second offset: its second pair is (-val1h, val2w), negated
when val1h > 0 or (val1h == 0 and val2w < 0) (mode 2), and (0, |val1w|) in modes 4-7; the integer path reads the pair as
it is. Float sums are ordered r1 + r2 + r3 + r4, so the pairing changes bits.
"""
from __future__ import annotations

import json
import math
from functools import lru_cache

import numpy as np

import fixtures as fx

M32 = 0xFFFFFFFF
F = np.float32
ALGO_OLD, ALGO_UNIFORM, ALGO_GAUSSIAN = 0, 1, 2
TV_Y = (16 << 8, 235 << 8)   # 4096 .. 60160
TV_C = (16 << 8, 240 << 8)   # 4096 .. 61440


# ---- the create-time checks (Data.setData, in its order), restated as data ----------------------------------------------
def _fmt(v) -> str:
    """Zig's {d}: integers without a point, floats in their shortest decimal form"""
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    v = float(v)
    return str(int(v)) if v == int(v) and abs(v) < 1e15 else repr(v)


ARRAY_CHECKS = [("thr", 3, 0, 255), ("thr1", 3, 0, 255), ("thr2", 3, 0, 255), ("grain", 2, 0, 127)]
SCALAR_CHECKS = [("sample_mode", 1, 7), ("range", 0, 255), ("angle_boost", 0, 65535), ("max_angle", 0, 1), ("random_param_ref", 0, 255),
                 ("random_param_grain", 0, 255), ("random_algo_ref", 0, 2), ("random_algo_grain", 0, 2)]
DEFAULTS = dict(thr=0.99, thr1=None, thr2=None, grain=0.0, sample_mode=2, range=15, seed=0, blur_first=True, dynamic_grain=False, keep_tv_range=False,
                angle_boost=1.5, max_angle=0.15, random_param_ref=1.0, random_param_grain=1.0, random_algo_ref=1, random_algo_grain=1)


def _array(key, v, max_len, lo, hi, default):
    if v is None:
        return list(default)
    a = [v] if np.isscalar(v) else list(v)
    if len(a) > max_len:
        raise ValueError(f'Deband: parameter "{key}" has too many elements (got {len(a)}, max {max_len}).')
    out = []
    for i in range(3):
        x = a[min(i, len(a) - 1)]
        if x < lo or x > hi:
            raise ValueError(f'Deband: parameter "{key}[{i}]={_fmt(float(x))}" out of range [{_fmt(lo)}..{_fmt(hi)}].')
        out.append(float(x))
    return out


def check_args(**kw) -> dict:
    """the wrapper's argument checks -> resolved arguments (8-bit scale arrays of three)"""
    bad = set(kw) - set(DEFAULTS)
    if bad:
        raise TypeError(f"unknown arguments {sorted(bad)}")
    a = dict(DEFAULTS, **kw)
    r = {}
    r["thr"] = _array("thr", a["thr"], 3, 0, 255, [0.99] * 3)
    r["thr1"] = _array("thr1", a["thr1"], 3, 0, 255, r["thr"])
    r["thr2"] = _array("thr2", a["thr2"], 3, 0, 255, r["thr"])
    r["grain"] = _array("grain", a["grain"], 2, 0, 127, [0.0] * 3)
    for key, lo, hi in SCALAR_CHECKS:
        v = a[key]
        if v < lo or v > hi:
            isint = key in ("sample_mode", "range", "random_algo_ref", "random_algo_grain")
            raise ValueError(f'Deband: parameter "{key}={_fmt(int(v) if isint else float(v))}" out of range [{_fmt(lo)}..{_fmt(hi)}].')
        r[key] = v
    for key in ("seed", "blur_first", "dynamic_grain", "keep_tv_range"):
        r[key] = a[key]
    r["dynamic_grain"] = bool(a["dynamic_grain"]) and (r["grain"][0] > 0 or r["grain"][1] > 0)
    return r


def scale_value(v, is_float: bool):
    """Data.scaleValue: 8-bit scale -> the clip's (16-bit integers, or f32 on [0, 1])"""
    if is_float:
        return [F(x / 255.0) for x in v]
    return [int(math.trunc(x * 65535.0 / 255.0 + 0.5)) for x in v]


# ---- random numbers -----------------------------------------------------------------------------------------------------
def _r2d(s: int) -> float:
    # the 52 mantissa bits m of a double in [1, 2): (1 + m / 2^52 - 1) * 2 - 1, whose first two steps are exact
    return float((s << 20) | (s >> 12)) * 2.0 ** -51 - 1.0


def _round_away(x: float) -> int:
    r = math.trunc(x)
    return r + (1 if x > 0 else -1) if abs(x - r) >= 0.5 else r


class Rng:
    """randOld / randUniform / randGaussian on one shared 32-bit state"""

    def __init__(self, state: int):
        self.s = state & M32

    def uniform(self) -> float:
        self.s = (1664525 * self.s + 1013904223) & M32
        return _r2d(self.s)

    def old(self) -> float:
        u = self.s
        t = ((((u << 13) & M32) ^ u) >> 17) ^ ((u << 13) & M32) ^ u
        self.s = (((32 * t) & M32) ^ t) & M32
        return _r2d(self.s)

    def gaussian(self, param: float) -> float:
        while True:
            while True:
                x, y = self.uniform(), self.uniform()
                r2 = x * x + y * y
                if r2 <= 1.0 and r2 != 0.0:
                    break
            v = param * y * math.sqrt(-2.0 * math.log(r2) / r2)
            if -1.0 < v < 1.0:
                return v

    def real(self, algo: int, param: float) -> float:
        return self.old() if algo == ALGO_OLD else (self.uniform() if algo == ALGO_UNIFORM else self.gaussian(param))

    def value(self, algo: int, rng: int, param: float) -> int:
        return _round_away(self.real(algo, param) * float(rng))

    def value_f32(self, algo: int, rng, param: float):
        return F(self.real(algo, param) * float(F(rng)))


def bulk_reals(r: Rng, algo: int, param: float, n: int) -> np.ndarray:
    """the next n values of Rng.real() as an array (what fills a grain buffer); advances r"""
    if n == 0:
        return np.empty(0, np.float64)
    if algo == ALGO_UNIFORM:
        st = lcg_stream(r.s, n)
        r.s = int(st[-1])
        return _r2d_v(st)
    if algo == ALGO_OLD:
        return np.array([r.old() for _ in np.arange(n)], np.float64)
    pairs = int(n * 1.5) + 64  # every attempt takes two uniform values, accepted or not
    while True:
        st = lcg_stream(r.s, 2 * pairs)
        u = _r2d_v(st)
        x, y = u[0::2], u[1::2]
        r2 = x * x + y * y
        ok = (r2 <= 1.0) & (r2 != 0.0)
        idx = np.flatnonzero(ok)
        lg = np.array([math.log(v) for v in r2[idx].tolist()], np.float64)  # (the C library's log, as Rng.gaussian)
        v = param * y[idx] * np.sqrt(-2.0 * lg / r2[idx])
        keep = (v > -1.0) & (v < 1.0)
        if int(keep.sum()) >= n:
            last = idx[keep][n - 1]
            r.s = int(st[2 * last + 1])
            return v[keep][:n]
        pairs *= 2


def lcg_stream(state: int, n: int) -> np.ndarray:
    """the next n states of randUniform, by doubling"""
    out = np.empty(max(n, 1), np.uint64)
    a, c = 1664525, 1013904223
    out[0] = (a * (state & M32) + c) & M32
    k = 1
    while k < n:
        m = min(k, n - k)
        out[k:k + m] = (out[:m] * np.uint64(a) + np.uint64(c)) & np.uint64(M32)
        a, c = (a * a) & M32, (a * c + c) & M32
        k += m
    return out[:n]


def _r2d_v(s: np.ndarray) -> np.ndarray:
    raw = ((s << np.uint64(20)) | (s >> np.uint64(12))) | np.uint64(0x3FF0000000000000)
    return (raw.view(np.float64) - 1.0) * 2.0 - 1.0


def _round_away_v(x: np.ndarray) -> np.ndarray:
    r = np.trunc(x)
    return (r + np.where(np.abs(x - r) >= 0.5, np.sign(x), 0.0)).astype(np.int64)


def ref_encode(t):
    """neo_f3kdb's signed char: truncate, abs, truncate again: 128 comes back as -128"""
    t = np.asarray(t, np.int64)
    a = np.abs(((t + 128) & 255) - 128)
    return np.where(a >= 128, a - 256, a)


def seed_mix(seed: int, width: int, height: int, num_frames: int) -> int:
    us = (0x92D68CA2 - (seed & M32)) & M32
    us ^= ((width << 16) & M32) ^ (height & M32)
    us ^= ((num_frames << 16) & M32) ^ (num_frames & M32)
    return us


def cur_range_grid(width: int, height: int, rng: int, mode: int) -> np.ndarray:
    x, y = np.arange(width), np.arange(height)
    xr = np.minimum(np.minimum(rng, x), width - 1 - x)[None, :]
    yr = np.minimum(np.minimum(rng, y), height - 1 - y)[:, None]
    if mode == 1:
        return np.broadcast_to(yr, (height, width)).copy()
    if mode == 3:
        return np.broadcast_to(xr, (height, width)).copy()
    return np.minimum(xr, yr)


def grain_items(width: int, height: int) -> int:
    return ((width + 255) & 0xFFFFFF80) * height


def tables(width, height, ssw=0, ssh=0, num_frames=1, range=15, sample_mode=2, seed=0, random_algo_ref=1, random_algo_grain=1, random_param_ref=1.0,
           random_param_grain=1.0, grain=(0, 0), dynamic_grain=False, is_float=False, fast=None) -> dict:
    """TempBuff.initFrameLuts. grain: the two strengths on the clip's scale. ->
    luma (h, w, 2) int8, chroma (ceil(h / 2^ssh), ceil(w / 2^ssw), 2) int8 (the luma entries at the chroma sites),
    grain_y / grain_c (items [x 3], int16 or f32; None for strength 0), grain_offsets (uint32 [num_frames] or None), max_offset."""
    w, h, mode = int(width), int(height), int(sample_mode)
    cr = cur_range_grid(w, h, int(range), mode)
    nref = np.where(cr > 0, 2 if mode == 2 else 1, 0)
    sited = ((np.arange(w) & ((1 << ssw) - 1)) == 0)[None, :] & ((np.arange(h) & ((1 << ssh) - 1)) == 0)[:, None]
    items = grain_items(w, h)
    total = items * (3 if dynamic_grain else 1)
    state = seed_mix(seed, w, h, num_frames)
    if fast is None:
        fast = random_algo_ref == ALGO_UNIFORM and random_algo_grain == ALGO_UNIFORM
    v1 = np.zeros((h, w), np.int64)
    v2 = np.zeros((h, w), np.int64)
    gbuf = [None, None]
    if fast:
        assert random_algo_ref == ALGO_UNIFORM and random_algo_grain == ALGO_UNIFORM
        per = 1 + nref + 2 * sited
        start = np.concatenate([[0], np.cumsum(per.ravel())])
        n_grid = int(start[-1])
        u = _r2d_v(lcg_stream(state, n_grid + 2 * total + (num_frames if dynamic_grain else 0)))
        first = (start[:-1] + 1).reshape(h, w)
        m = cr > 0
        v1[m] = ref_encode(_round_away_v(u[first[m]] * cr[m]))
        if mode == 2:
            v2[m] = ref_encode(_round_away_v(u[first[m] + 1] * cr[m]))
        pos = n_grid
        for i in (0, 1):
            if grain[i] > 0:
                g = u[pos:pos + total]
                gbuf[i] = (g * float(F(grain[i]))).astype(F) if is_float else _round_away_v(g * float(int(grain[i]))).astype(np.int16)
            pos += total
        offs = None
        if dynamic_grain:
            o = (items + _round_away_v(u[pos:pos + num_frames] * float(items))) & 0xFFFFFFF0
            offs = o.astype(np.uint32)
    else:
        r = Rng(state)
        ar, ag, pr, pg = random_algo_ref, random_algo_grain, float(random_param_ref), float(random_param_grain)
        crl, sl = cr.tolist(), sited.tolist()
        for y in np.arange(h).tolist():
            for x in np.arange(w).tolist():
                r.real(ag, pg)
                c = crl[y][x]
                if c > 0:
                    v1[y, x] = r.value(ar, c, pr)
                    if mode == 2:
                        v2[y, x] = r.value(ar, c, pr)
                if sl[y][x]:
                    r.real(ag, pg)
                    r.real(ag, pg)
        v1, v2 = ref_encode(v1), ref_encode(v2)
        for i in (0, 1):
            if grain[i] > 0:
                g = bulk_reals(r, ag, pg, total)
                gbuf[i] = (g * float(F(grain[i]))).astype(F) if is_float else _round_away_v(g * float(int(grain[i]))).astype(np.int16)
            else:
                bulk_reals(r, ag, pg, total)
        offs = None
        if dynamic_grain:
            offs = np.array([(items + r.value(ALGO_UNIFORM, items, 1.0)) & 0xFFFFFFF0 for _ in np.arange(num_frames)], np.uint32)
    luma = np.stack([v1, v2], -1).astype(np.int8)
    chroma = np.ascontiguousarray(luma[::1 << ssh, ::1 << ssw])
    return dict(luma=luma, chroma=chroma, grain_y=gbuf[0], grain_c=gbuf[1], grain_offsets=offs, max_offset=int(np.abs(luma.astype(np.int64)).max(initial=0)),
                items=items)


# ---- the polynomial routines of src/vcl.zig, operation by operation ---------------------------------------------------------
def _fma(a, b, c):
    from oracle import vs_host as vh

    return vh.fma32(a, b, c).astype(F)


def _round32(x):
    x = np.asarray(x, F)
    r = np.trunc(x)
    return (r + np.where(np.abs(x - r) >= F(0.5), np.copysign(F(1), x), F(0))).astype(F)


def vcl_atan(x):
    x = np.asarray(x, F)
    P3, P2, P1, P0 = F(8.05374449538E-2), F(-1.38776856032E-1), F(1.99777106478E-1), F(-3.33329491539E-1)
    pi_2, pi_4, sqrt2 = F(math.pi * 0.5), F(math.pi * 0.25), F(math.sqrt(2.0))
    t = np.abs(x)
    notsmal = t >= F(sqrt2 - F(1.0))
    notbig = t <= F(sqrt2 + F(1.0))
    s = np.where(notbig, pi_4, pi_2).astype(F)
    s = np.where(notsmal, s, F(0)).astype(F)
    a = np.where(notbig, t, F(0)).astype(F)
    a = (a + np.where(notsmal, F(-1), F(0)).astype(F)).astype(F)
    b = np.where(notbig, F(1), F(0)).astype(F)
    b = (b + np.where(notsmal, t, F(0)).astype(F)).astype(F)
    z = (a / b).astype(F)
    zz = (z * z).astype(F)
    z2 = (zz * zz).astype(F)
    re = _fma(_fma(P3, zz, P2), z2, _fma(P1, zz, P0))  # polynomial_3(zz, P0, P1, P2, P3)
    re = (_fma(re, (zz * z).astype(F), z) + s).astype(F)
    return np.copysign(np.abs(re), x).astype(F)


def vcl_pow(x0, y):
    x0 = np.asarray(x0, F)
    y = F(y)
    ln2f_hi, ln2f_lo, ln2, log2e, sqrt2_half = F(0.693359375), F(-2.12194440e-4), F(0.6931471805599453), F(1.4426950408889634), F(0.7071067811865476)
    P = [F(v) for v in (3.3333331174E-1, -2.4999993993E-1, 2.0000714765E-1, -1.6668057665E-1, 1.4249322787E-1, -1.2420140846E-1, 1.1676998740E-1,
                        -1.1514610310E-1, 7.0376836292E-2)]
    E = [F(1.0 / 2.0), F(1.0 / 6.0), F(1.0 / 24.0), F(1.0 / 120.0), F(1.0 / 720.0), F(1.0 / 5040.0)]
    half, one = F(0.5), F(1.0)
    x1 = np.abs(x0)
    bits = x1.view(np.uint32)
    x = ((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(F)  # fraction_2
    blend = x > sqrt2_half
    x = np.where(blend, x, (x + x).astype(F)).astype(F)
    x = (x - one).astype(F)
    x2 = (x * x).astype(F)
    x4 = (x2 * x2).astype(F)
    x8 = (x4 * x4).astype(F)
    lg1 = _fma(_fma(_fma(P[7], x, P[6]), x2, _fma(P[5], x, P[4])), x4,
               _fma(_fma(P[3], x, P[2]), x2, (_fma(P[1], x, P[0]) + (P[8] * x8).astype(F)).astype(F)))  # polynomial_8
    lg1 = (lg1 * (x2 * x).astype(F)).astype(F)
    ef = (((bits >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int32) - 127).astype(F)  # exponent_f
    ef = np.where(blend, (ef + one).astype(F), ef).astype(F)
    e1 = _round32((ef * y).astype(F))
    yr = _fma(ef, y, -e1)
    lg = (_fma(half, -x2, x) + lg1).astype(F)
    x2err = _fma((half * x).astype(F), x, (half * -x2).astype(F))
    lgerr = (_fma(half, x2, (lg - x).astype(F)) - lg1).astype(F)
    e2 = _round32(((lg * y).astype(F) * log2e).astype(F))
    v = _fma(lg, y, (-e2 * ln2f_hi).astype(F))
    v = _fma(-e2, ln2f_lo, v)
    corr = _fma((lgerr + x2err).astype(F), y, (-yr * ln2).astype(F))
    v = (v - corr).astype(F)
    x = v
    e3 = _round32((x * log2e).astype(F))
    x = _fma(-e3, ln2, x)
    x2e = (x * x).astype(F)
    xx4 = (x2e * x2e).astype(F)
    z = _fma(_fma(E[3], x, E[2]), x2e, _fma(_fma(E[5], x, E[4]), xx4, _fma(E[1], x, E[0])))  # polynomial_5
    z = (((z * x2e).astype(F) + x).astype(F) + one).astype(F)
    ee = ((e1 + e2).astype(F) + e3).astype(F)
    ei = _round32(ee).astype(np.int64)
    zb = (z.view(np.uint32).astype(np.int64) + (ei << 23)) & M32
    z = zb.astype(np.uint32).view(F)
    xzero = (x0.view(np.uint32) & np.uint32(0x7F800000)) == 0
    zero_case = F(np.inf) if y < 0 else (one if y == 0 else F(0))
    return np.where(xzero, zero_case, z).astype(F)


# ---- processPlane -------------------------------------------------------------------------------------------------------
def gradient_angle(src: np.ndarray, rd: int = 20) -> np.ndarray:
    """calculateGradientAngle at every sample of the plane: a Sobel at distance rd, coordinates clamped to the plane"""
    h, w = src.shape
    s = src.astype(F)
    ys, xs = np.arange(h), np.arange(w)
    cy = lambda d: np.clip(ys + d, 0, h - 1)
    cx = lambda d: np.clip(xs + d, 0, w - 1)
    at = lambda dy, dx: s[np.ix_(cy(dy), cx(dx))]
    p00, p10, p20 = at(-rd, -rd), at(-rd, 0), at(-rd, rd)
    p01, p21 = at(0, -rd), at(0, rd)
    p02, p12, p22 = at(rd, -rd), at(rd, 0), at(rd, rd)
    two = F(2)
    gx = (((p20 + two * p21).astype(F) + p22).astype(F) - ((p00 + two * p01).astype(F) + p02).astype(F)).astype(F)
    gy = (((p00 + two * p10).astype(F) + p20).astype(F) - ((p02 + two * p12).astype(F) + p22).astype(F)).astype(F)
    small = np.abs(gx) < F(0.01 * 3.0)
    with np.errstate(all="ignore"):
        ang = ((vcl_atan((gy / gx).astype(F)) / F(math.pi)).astype(F) + F(0.5)).astype(F)
    return np.where(small, F(1), ang).astype(F)


def plane_offsets(off: np.ndarray, ssw: int, ssh: int, mode: int, is_float: bool):
    """(dy1, dx1, dy2, dx2) per sample from the (val1, val2) pairs: refs 1 / 3 at +-(dy1, dx1), refs 2 / 4 at +-(dy2, dx2)"""
    v1, v2 = off[..., 0].astype(np.int64), off[..., 1].astype(np.int64)
    v1w, v1h, v2w, v2h = v1 >> ssw, v1 >> ssh, v2 >> ssw, v2 >> ssh
    z = np.zeros_like(v1)
    if mode == 1:
        return v1h, z, z, z
    if mode == 3:
        return z, v1w, z, z
    if mode == 2:
        dy2, dx2 = -v1h, v2w
        if is_float:
            neg = (v1h > 0) | ((v1h == 0) & (v2w < 0))
            dy2, dx2 = np.where(neg, -dy2, dy2), np.where(neg, -dx2, dx2)
        return v2h, v1w, dy2, dx2
    return v1h, z, z, (np.abs(v1w) if is_float else v1w)


def boost_mask(src, off, ssw, ssh, max_angle) -> np.ndarray:
    """mode 7: where max_angle_diff <= max_angle"""
    h, w = src.shape
    ang = gradient_angle(src)
    v1 = off[..., 0].astype(np.int64)
    yo, xo = v1 >> ssh, v1 >> ssw
    yy, xx = np.mgrid[0:h, 0:w]
    a0 = ang
    d = lambda a: np.abs((a - a0).astype(F))
    m = np.maximum(d(ang[yy + yo, xx]), d(ang[yy - yo, xx]))
    m = np.maximum(m, np.maximum(d(ang[yy, xx + xo]), d(ang[yy, xx - xo])))
    return m <= F(max_angle)


def deband_plane(src, off, ssw=0, ssh=0, grain=None, thr=0, thr1=None, thr2=None, lo=None, hi=None, sample_mode=2, blur_first=True, angle_boost=1.5,
                 max_angle=0.15) -> np.ndarray:
    """processPlane on one plane. off: (h, w, 2) int8 pairs of this plane's table; grain: (h, w) int16 / f32 or None;
    thr / thr1 / thr2 and the clamp lo / hi on the plane's scale."""
    h, w = src.shape
    mode = int(sample_mode)
    is_float = src.dtype == np.float32
    assert is_float or src.dtype == np.uint16
    thr1 = thr if thr1 is None else thr1
    thr2 = thr if thr2 is None else thr2
    dy1, dx1, dy2, dx2 = plane_offsets(off[:h, :w], ssw, ssh, mode, is_float)
    yy, xx = np.mgrid[0:h, 0:w]
    s = src.astype(F) if is_float else src.astype(np.int64)
    r1, r3 = s[yy + dy1, xx + dx1], s[yy - dy1, xx - dx1]
    four = mode not in (1, 3)
    if four:
        r2, r4 = s[yy + dy2, xx + dx2], s[yy - dy2, xx - dx2]
    c = s
    boost = boost_mask(src, off[:h, :w], ssw, ssh, max_angle) if mode == 7 else None
    if is_float:
        t, t1, t2 = F(thr), F(thr1), F(thr2)
        ad = lambda a: np.abs((a - c).astype(F))
        if mode in (1, 3):
            avg = ((r1 + r3).astype(F) * F(0.5)).astype(F)
            orig = (ad(avg) >= t) if blur_first else ((ad(r1) >= t) | (ad(r3) >= t))
            out = np.where(orig, c, avg)
        elif mode == 2:
            avg = ((((r1 + r2).astype(F) + r3).astype(F) + r4).astype(F) * F(0.25)).astype(F)
            orig = (ad(avg) >= t) if blur_first else ((ad(r1) >= t) | (ad(r2) >= t) | (ad(r3) >= t) | (ad(r4) >= t))
            out = np.where(orig, c, avg)
        elif mode == 4:
            av, ah = ((r1 + r3).astype(F) * F(0.5)).astype(F), ((r2 + r4).astype(F) * F(0.5)).astype(F)
            ov = (ad(av) >= t) if blur_first else ((ad(r1) >= t) | (ad(r3) >= t))
            oh = (ad(ah) >= t) if blur_first else ((ad(r2) >= t) | (ad(r4) >= t))
            out = ((np.where(ov, c, av) + np.where(oh, c, ah)).astype(F) * F(0.5)).astype(F)
        elif mode == 5:
            avg = ((((r1 + r2).astype(F) + r3).astype(F) + r4).astype(F) * F(0.25)).astype(F)
            mx = np.maximum(np.maximum(ad(r1), ad(r2)), np.maximum(ad(r3), ad(r4)))
            two = (c * F(2)).astype(F)
            m1, m2 = np.abs(((r1 + r3).astype(F) - two).astype(F)), np.abs(((r2 + r4).astype(F) - two).astype(F))
            orig = (ad(avg) >= t) | (mx >= t1) | (m1 >= t2) | (m2 >= t2)
            out = np.where(orig, c, avg)
        else:
            out = _soft(c, r1, r3, r2, r4, t, t1, t2, boost, angle_boost)
        out = out.astype(F)
        if grain is not None:
            out = (out + grain.astype(F)).astype(F)
        lo = F(0) if lo is None else F(lo)
        hi = F(1) if hi is None else F(hi)
        return np.fmax(lo, np.fmin(out, hi)).astype(F)
    t, t1, t2 = int(thr), int(thr1), int(thr2)
    ad = lambda a: np.abs(a - c)
    if mode in (1, 3):
        avg = (r1 + r3 + 1) >> 1
        orig = (ad(avg) >= t) if blur_first else ((ad(r1) >= t) | (ad(r3) >= t))
        out = np.where(orig, c, avg)
    elif mode == 2:
        a1, a2 = (r1 + r3 + 1) >> 1, (r2 + r4 + 1) >> 1
        a1 = a1 - (a1 > 0)
        avg = (a1 + a2 + 1) >> 1
        orig = (ad(avg) >= t) if blur_first else ((ad(r1) >= t) | (ad(r2) >= t) | (ad(r3) >= t) | (ad(r4) >= t))
        out = np.where(orig, c, avg)
    elif mode == 4:
        av, ah = (r1 + r3 + 1) >> 1, (r2 + r4 + 1) >> 1
        ov = (ad(av) >= t) if blur_first else ((ad(r1) >= t) | (ad(r3) >= t))
        oh = (ad(ah) >= t) if blur_first else ((ad(r2) >= t) | (ad(r4) >= t))
        out = (np.where(ov, c, av) + np.where(oh, c, ah) + 1) >> 1
    elif mode == 5:
        avg = (r1 + r3 + r2 + r4) >> 2
        mx = np.maximum(np.maximum(ad(r1), ad(r3)), np.maximum(ad(r2), ad(r4)))
        m1, m2 = np.abs((r1 + r3) - 2 * c), np.abs((r2 + r4) - 2 * c)
        orig = (ad(avg) >= t) | (mx >= t1) | (m1 >= t2) | (m2 >= t2)
        out = np.where(orig, c, avg)
    else:
        f = lambda a: a.astype(F)
        bl = _soft(f(c), f(r1), f(r3), f(r2), f(r4), F(t), F(t1), F(t2), boost, angle_boost)
        out = np.trunc((bl + F(0.5)).astype(F)).astype(np.int64)
    if grain is not None:
        out = out + grain.astype(np.int64)
    lo = 0 if lo is None else int(lo)
    hi = 65535 if hi is None else int(hi)
    return np.clip(out, lo, hi).astype(np.uint16)


def _soft(c, p1, p2, p3, p4, t_avg, t_max, t_mid, boost, angle_boost):
    """modes 6 and 7 (p1, p2: the first pair; p3, p4: the second): src + (avg - src) * pow(product of four soft thresholds, 0.1)"""
    shape = c.shape
    t_avg, t_max, t_mid = (np.full(shape, v, F) for v in (t_avg, t_max, t_mid))
    if boost is not None:
        ab = F(angle_boost)
        t_avg, t_max, t_mid = (np.where(boost, (v * ab).astype(F), v).astype(F) for v in (t_avg, t_max, t_mid))
    avg = ((((p1 + p2).astype(F) + p3).astype(F) + p4).astype(F) * F(0.25)).astype(F)
    diff = (avg - c).astype(F)
    ad = lambda a: np.abs((a - c).astype(F))
    mx = np.maximum(np.maximum(ad(p1), ad(p2)), np.maximum(ad(p3), ad(p4)))
    two = (c * F(2)).astype(F)
    mv, mh = np.abs(((p1 + p2).astype(F) - two).astype(F)), np.abs(((p3 + p4).astype(F) - two).astype(F))
    eps = F(1e-5)
    sat = lambda v: np.maximum(F(0), np.minimum(v, F(1))).astype(F)
    comp = lambda d, t: sat((F(3) * (F(1) - (d / np.maximum(t, eps)).astype(F)).astype(F)).astype(F))
    prod = (((comp(np.abs(diff), t_avg) * comp(mx, t_max)).astype(F) * comp(mv, t_mid)).astype(F) * comp(mh, t_mid)).astype(F)
    factor = vcl_pow(prod, F(0.1))
    return (c + (diff * factor).astype(F)).astype(F)


# ---- the wrapper on one frame ---------------------------------------------------------------------------------------------
def grain_pitch(width: int, itemsize: int, align: int = 32) -> int:
    n = align // itemsize
    return (width + n - 1) // n * n


def grain_plane(buf: np.ndarray, offset: int, pitch: int, h: int, w: int) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return buf[offset + yy * pitch + xx]


def deband_frame(planes, family="GRAY", ssw=0, ssh=0, n=0, num_frames=1, align=32, tab=None, **kw) -> list:
    """vszip.Deband on frame n of a clip of num_frames frames of this geometry; family "GRAY" | "YUV" | "RGB". `tab`: tables()
    of the clip made before (they depend on the clip, not on the frame)."""
    a = check_args(**kw)
    is_float = planes[0].dtype == np.float32
    h, w = planes[0].shape
    thr, thr1, thr2, gr = (scale_value(a[k], is_float) for k in ("thr", "thr1", "thr2", "grain"))
    if tab is None:
        tab = clip_tables(w, h, ssw, ssh, num_frames, is_float, a)
    yuv = family == "YUV"
    out = []
    for i, p in enumerate(planes):
        if is_float:
            lo, hi = ((-0.5, 0.5) if i > 0 else (0.0, 1.0)) if yuv else (0.0, 1.0)
        elif a["keep_tv_range"] and yuv:
            lo, hi = TV_C if i > 0 else TV_Y
        else:
            lo, hi = 0, 65535
        buf = tab["grain_y"] if i == 0 else tab["grain_c"]
        g = None
        if buf is not None:
            off = int(tab["grain_offsets"][n]) if tab["grain_offsets"] is not None else 0
            g = grain_plane(buf, off, grain_pitch(w if i == 0 else (w >> ssw), p.dtype.itemsize, align), p.shape[0], p.shape[1])
        t = tab["luma"] if i == 0 else tab["chroma"]
        out.append(deband_plane(p, t, ssw if i > 0 else 0, ssh if i > 0 else 0, g, thr[i], thr1[i], thr2[i], lo, hi, a["sample_mode"], a["blur_first"],
                                a["angle_boost"], a["max_angle"]))
    return out


def clip_tables(w, h, ssw, ssh, num_frames, is_float, a) -> dict:
    gr = scale_value(a["grain"], is_float)
    return tables(w, h, ssw, ssh, num_frames, a["range"], a["sample_mode"], a["seed"], a["random_algo_ref"], a["random_algo_grain"], a["random_param_ref"],
                  a["random_param_grain"], (gr[0] if a["grain"][0] > 0 else 0, gr[1] if a["grain"][1] > 0 else 0), a["dynamic_grain"], is_float)


# ---- the reference's golden cases (tests/goldens/deband.json), rebuilt from tests/fixtures.py ------------------------------
_FMT = {  # name -> (family, bits, ssw, ssh, float)
    "GRAY8": ("GRAY", 8, 0, 0, False), "GRAY16": ("GRAY", 16, 0, 0, False), "GRAYS": ("GRAY", 32, 0, 0, True), "YUV420P8": ("YUV", 8, 1, 1, False),
    "YUV420P16": ("YUV", 16, 1, 1, False), "YUV422P8": ("YUV", 8, 1, 0, False), "YUV422P16": ("YUV", 16, 1, 0, False), "YUV444PS": ("YUV", 32, 0, 0, True),
    "RGB48": ("RGB", 16, 0, 0, False), "RGBS": ("RGB", 32, 0, 0, True),
}
# keys the spec does not rebuild, each with its reason (tests/test_deband_ref.py asserts this is exactly what it leaves out)
LEFT_OUT = {
    "GRAY8|full|grain=16,seed=7,thr=48": "8-bit clip: passes through the host resizer (to 16 bits, and error-diffusion dither back) around the filter",
    "YUV420P8|full|grain=16,seed=7,thr=48": "8-bit clip: passes through the host resizer around the filter",
    "YUV422P8|full|grain=[16,8],seed=7,thr=[48,24]": "8-bit clip: passes through the host resizer around the filter",
}


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "deband_goldens.json").read_text())


def parse_key(key: str):
    """'YUV420P16|full|grain=[16,8],seed=7,thr=[48,24]' -> (format, geometry, keyword arguments)"""
    fmt, geometry, args = key.split("|")
    kw, depth, item, items = {}, 0, "", []
    for ch in args + ",":
        if ch == "," and depth == 0:
            items.append(item)
            item = ""
            continue
        depth += (ch == "[") - (ch == "]")
        item += ch
    num = lambda s: float(s) if "." in s else int(s)
    for it in items:
        k, v = it.split("=")
        kw[k] = [num(x) for x in v[1:-1].split(",")] if v.startswith("[") else num(v)
    for k in ("blur_first", "dynamic_grain", "keep_tv_range"):
        if k in kw:
            kw[k] = bool(kw[k])
    return fmt, geometry, kw


@lru_cache(maxsize=None)
def _planes(fmt: str, geometry: str) -> tuple:
    family, bits, ssw, ssh, flt = _FMT[fmt]
    if family == "YUV":
        p = fx.yuv_geometry(fx.crop_yuv(bits, ssw, ssh, sample="f32") if flt else fx.crop_yuv(bits, ssw, ssh), geometry, ssw, ssh)
    elif family == "RGB":
        assert geometry == "full"
        p = [np.ascontiguousarray(c) for c in (fx.crop_rgbs() if flt else fx.crop_rgb24().astype(np.uint16) * np.uint16(257))]
    else:
        g = fx.crop_grays() if flt else fx.crop_gray16()
        g = g if geometry == "full" else (g[:-1, :-1] if geometry == "odd" else g[100:107, 200:213])
        p = [np.ascontiguousarray(g)]
    for x in p:
        x.setflags(write=False)
    return tuple(p)


def golden_inputs(fmt: str, geometry: str) -> list:
    return list(_planes(fmt, geometry))


def run_key(key: str, align: int = 32) -> list:
    fmt, geometry, kw = parse_key(key)
    family, bits, ssw, ssh, flt = _FMT[fmt]
    assert bits >= 16
    return deband_frame(golden_inputs(fmt, geometry), family, ssw, ssh, align=align, **kw)


@lru_cache(maxsize=None)
def banded16() -> np.ndarray:
    """the reference's behavioural fixture: the GRAY16 crop bit-crushed to 256 levels by two point conversions (zimg's
    limited-range depth conversion without dither: 16 -> 8 is x / 256 rounded half to even, 8 -> 16 is x * 256)"""
    g8 = np.clip(np.rint(fx.crop_gray16().astype(F) * F(1.0 / 256.0)), 0, 255).astype(np.uint16)
    a = (g8 << np.uint16(8)).astype(np.uint16)
    a.setflags(write=False)
    return a
