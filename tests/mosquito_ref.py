"""CPU parity spec of MosquitoNR (the reference's src/filters/mosquito_nr.zig and mosquito_nr_float.zig with the
create-time rules of src/vapoursynth/mosquito_nr.zig): a numpy restatement that reproduces every key of the reference's
tests/goldens/mosquito.json from tests/fixtures.py's inputs (tests/test_mosquito_ref.py).
tests/test_gpu_mosquito.py checks vszip_mosquito_nr against it bit for bit, float included.

One algorithm in three working types: wrapping 16-bit for 8-bit samples, 32-bit for 9..16-bit samples, IEEE f32 with no
contraction for float samples. `work` selects another integer width for the 8-bit form (the spec's own cross-check that
nothing wraps: tests/test_mosquito_ref.py).

Not part of oracle/ (frozen): a test-support module like fixtures.py.
"""
from __future__ import annotations

import json
from functools import lru_cache

import numpy as np

import fixtures as fx
from combmask_ref import _crop_gray

NAME = "MosquitoNR"


# ---- the create-time checks ---------------------------------------------------------------------------------------------
def expand3(v, default: int) -> tuple:
    """hz.getArray: up to three values, a missing first one is the default, later ones repeat the one before.
    -> (the values as given, the three per-plane values)"""
    vals = [int(v)] if isinstance(v, (int, np.integer)) else ([] if v is None else [int(x) for x in v])
    out = []
    for i in range(3):
        out.append(vals[i] if i < len(vals) else (default if i == 0 else out[i - 1]))
    return vals, out


def _check_array(key: str, v, default: int, lo: int, hi: int) -> list:
    vals, out = expand3(v, default)
    if len(vals) > 3:
        raise ValueError(f"{NAME}: {key} has too many elements (got {len(vals)}, max 3).")
    for x in out:
        if x < lo:
            raise ValueError(f"{NAME}: {key} value {x} is below minimum {lo}.")
        if x > hi:
            raise ValueError(f"{NAME}: {key} value {x} is above maximum {hi}.")
    return out


def check_mosquito_args(sizes, strength=16, restore=128, radius=2) -> tuple:
    """mosquitoNRCreate's checks, in its order; ValueError with its wording. sizes: (h, w) of every PROCESSED plane.
    -> the three per-plane arrays (strength, restore, radius)"""
    if any(w < 4 or h < 4 for h, w in sizes):
        raise ValueError(f"{NAME}: input is too small (need at least 4x4 per processed plane).")
    return (_check_array("strength", strength, 16, 0, 32), _check_array("restore", restore, 128, 0, 128), _check_array("radius", radius, 2, 1, 2))


# ---- arithmetic in the working type -------------------------------------------------------------------------------------
class _Int:
    """two's complement of `width` bits: every result is wrapped, as the reference's +% and -% do"""

    def __init__(self, width: int):
        self.width = width

    def w(self, v):
        m = 1 << self.width
        return ((np.asarray(v, np.int64) + (m >> 1)) & (m - 1)) - (m >> 1)

    def add(self, a, b):
        return self.w(a + b)

    def sub(self, a, b):
        return self.w(a - b)

    def half(self, a):
        return a >> 1

    def quarter(self, a):
        return a >> 2

    def absv(self, v):
        return np.maximum(v, self.w(-v))


class _Flt:
    def add(self, a, b):
        return a + b

    def sub(self, a, b):
        return a - b

    def half(self, a):
        return a * np.float32(0.5)

    def quarter(self, a):
        return a * np.float32(0.25)

    def absv(self, v):
        return np.abs(v)


# The eight directions. A SAD term is one neighbour (dx, dy) or the average of two; a blur is over `near` (weight
# strength) and, for the half-way directions of radius 2, `far` (weight 2 strength). Orders are the reference's.
_SAD = {
    1: [[(-1, 0), (1, 0)], [(-1, -1), (1, 1)], [(0, -1), (0, 1)], [(1, -1), (-1, 1)],
        [((-1, 0), (-1, -1)), ((1, 0), (1, 1))], [((-1, -1), (0, -1)), ((1, 1), (0, 1))],
        [((0, -1), (1, -1)), ((0, 1), (-1, 1))], [((1, 0), (1, -1)), ((-1, 0), (-1, 1))]],
    2: [[(-1, 0), (1, 0), (-2, 0), (2, 0)], [(-1, -1), (1, 1), (-2, -2), (2, 2)], [(0, -1), (0, 1), (0, -2), (0, 2)], [(1, -1), (-1, 1), (2, -2), (-2, 2)],
        [(-2, -1), (2, 1), ((-1, 0), (-1, -1)), ((1, 0), (1, 1))], [(-1, -2), (1, 2), ((-1, -1), (0, -1)), ((1, 1), (0, 1))],
        [(1, -2), (-1, 2), ((0, -1), (1, -1)), ((0, 1), (-1, 1))], [(2, -1), (-2, 1), ((1, -1), (1, 0)), ((-1, 1), (-1, 0))]],
}
_NEAR = {
    1: [[(-1, 0), (1, 0)], [(-1, -1), (1, 1)], [(0, -1), (0, 1)], [(1, -1), (-1, 1)],
        [(-1, -1), (-1, 0), (1, 0), (1, 1)], [(-1, -1), (0, -1), (0, 1), (1, 1)], [(1, -1), (0, -1), (0, 1), (-1, 1)], [(1, -1), (1, 0), (-1, 0), (-1, 1)]],
    2: [[(-2, 0), (-1, 0), (1, 0), (2, 0)], [(-2, -2), (-1, -1), (1, 1), (2, 2)], [(0, -2), (0, -1), (0, 1), (0, 2)], [(2, -2), (1, -1), (-1, 1), (-2, 2)],
        [(-1, -1), (-1, 0), (1, 0), (1, 1)], [(-1, -1), (0, -1), (0, 1), (1, 1)], [(1, -1), (0, -1), (0, 1), (-1, 1)], [(1, -1), (1, 0), (-1, 0), (-1, 1)]],
}
_FAR = [[(-2, -1), (2, 1)], [(-1, -2), (1, 2)], [(1, -2), (-1, 2)], [(2, -1), (-2, 1)]]  # directions 4 .. 7 of radius 2


def _lift_fwd(op, x):
    """one level of the 5/3 lifting along axis 0 -> (approximation, detail)"""
    n = x.shape[0]
    na, nd = (n + 1) // 2, n // 2
    even, odd = x[0::2], x[1::2]
    right = even[np.minimum(np.arange(nd) + 1, na - 1)]  # sample 2 j + 2, or n - 2 beyond the end
    d = op.sub(odd, op.half(op.add(even[:nd], right)))
    j = np.arange(na)
    a = op.add(even, op.quarter(op.add(d[np.maximum(j - 1, 0)], d[np.minimum(j, nd - 1)])))
    return a, d


def _lift_inv(op, a, d):
    na, nd = a.shape[0], d.shape[0]
    j = np.arange(na)
    even = op.sub(a, op.quarter(op.add(d[np.maximum(j - 1, 0)], d[np.minimum(j, nd - 1)])))
    right = even[np.minimum(np.arange(nd) + 1, na - 1)]
    odd = op.add(d, op.half(op.add(even[:nd], right)))
    out = np.empty((na + nd,) + a.shape[1:], a.dtype)
    out[0::2], out[1::2] = even, odd
    return out


def intermediates(plane: np.ndarray, strength: int = 16, restore: int = 128, radius: int = 2, bits=None, chroma: bool = False, work=None) -> dict:
    """per-sample values of a processed plane (strength > 0): `dir` (0 .. 7, 8 = flat), `blur`, and `pre`, the value before
    the output clamp (integers: after the rounding shift by 4). Integers come back as int64, floats as float32.
    work: the integer working width (default 16 for 8-bit samples, 32 otherwise)."""
    assert plane.ndim == 2 and plane.dtype in (np.uint8, np.uint16, np.float32) and strength > 0
    h, w = plane.shape
    flt = plane.dtype == np.float32
    if flt:
        op, o = _Flt(), plane
    else:
        op = _Int(work or (16 if plane.dtype == np.uint8 else 32))
        o = op.w(plane.astype(np.int64) << 4)
    P = np.pad(o, 2, "reflect")
    N = lambda d: P[2 + d[1]:2 + d[1] + h, 2 + d[0]:2 + d[0] + w]
    c = o

    def term(t):
        v = op.half(op.add(N(t[0]), N(t[1]))) if isinstance(t[0], tuple) else N(t)
        return op.absv(op.sub(v, c))

    best, bi = None, np.zeros((h, w), np.int64)
    for k, terms in enumerate(_SAD[radius]):
        s = term(terms[0])
        for t in terms[1:]:
            s = op.add(s, term(t))
        if k == 0:
            best = s
        else:
            lt = s < best
            bi = np.where(lt, k, bi)
            best = np.where(lt, s, best)
    dirs = np.where(best == 0, 8, bi)

    def chain(offs):
        s = N(offs[0])
        for d in offs[1:]:
            s = s + N(d)  # integers: in 32 bits, no wrap; floats: left to right
        return s

    blur = c.copy()
    if flt:
        s = np.float32(strength)
        coef0, coef1 = (np.float32(64) - 2 * s, np.float32(128) - 4 * s) if radius == 1 else (np.float32(128) - 4 * s, np.float32(256) - 8 * s)
        inv_lo, inv_hi = (np.float32(1 / 64), np.float32(1 / 128)) if radius == 1 else (np.float32(1 / 128), np.float32(1 / 256))
        for k in range(8):
            if k < 4:
                v = (coef0 * c + s * chain(_NEAR[radius][k])) * inv_lo
            elif radius == 1:
                v = (coef1 * c + s * chain(_NEAR[1][k])) * inv_hi
            else:
                v = (coef1 * c + (2 * s) * chain(_FAR[k - 4]) + s * chain(_NEAR[2][k])) * inv_hi
            assert v.dtype == np.float32
            blur = np.where(dirs == k, v, blur)
    else:
        s = strength
        coef0, coef1 = (64 - 2 * s, 128 - 4 * s) if radius == 1 else (128 - 4 * s, 256 - 8 * s)
        sh = 6 if radius == 1 else 7
        for k in range(8):
            if k < 4:
                v = (coef0 * c + s * chain(_NEAR[radius][k]) + (1 << (sh - 1))) >> sh
            elif radius == 1:
                v = (coef1 * c + s * chain(_NEAR[1][k]) + (1 << sh)) >> (sh + 1)
            else:
                v = (coef1 * c + 2 * s * chain(_FAR[k - 4]) + s * chain(_NEAR[2][k]) + (1 << sh)) >> (sh + 1)
            blur = np.where(dirs == k, op.w(v), blur)

    out = blur
    if restore != 0:
        va_o, _ = _lift_fwd(op, o)
        ll_o, _ = _lift_fwd(op, va_o.T)
        va_b, vd_b = _lift_fwd(op, blur)
        ll_b, hd_b = _lift_fwd(op, va_b.T)
        ll = ll_o
        if restore != 128:
            if flt:
                wo = np.float32(restore) / np.float32(128)
                wb = np.float32(1) - wo
                ll = wo * ll_o + wb * ll_b
            else:
                ll = op.w((restore * ll_o + (128 - restore) * ll_b + 64) >> 7)
        va_rec = _lift_inv(op, ll, hd_b).T
        out = _lift_inv(op, va_rec, vd_b)
    pre = out if flt else op.add(out, 8) >> 4
    return {"dir": dirs, "blur": blur, "pre": pre}


def mosquito_nr(plane: np.ndarray, strength: int = 16, restore: int = 128, radius: int = 2, bits=None, chroma: bool = False, work=None) -> np.ndarray:
    """one 2-D plane (uint8, uint16 with `bits` 9 .. 16, or float32) with its own parameters"""
    assert plane.ndim == 2
    check_mosquito_args([plane.shape], strength, restore, radius)
    if plane.dtype == np.float32:
        if strength == 0:
            return plane.copy()
        lo, hi = (np.float32(-0.5), np.float32(0.5)) if chroma else (np.float32(0), np.float32(1))
        return np.minimum(np.maximum(intermediates(plane, strength, restore, radius, None, chroma)["pre"], lo), hi).astype(np.float32)
    bits = bits if bits is not None else 8 * plane.dtype.itemsize
    assert (plane.dtype == np.uint8 and bits == 8) or (plane.dtype == np.uint16 and 9 <= bits <= 16), (plane.dtype, bits)
    if strength == 0:
        return plane.copy()
    return np.clip(intermediates(plane, strength, restore, radius, bits, chroma, work)["pre"], 0, (1 << bits) - 1).astype(plane.dtype)


def mosquito_frame(planes, strength=16, restore=128, radius=2, which=(0,), bits=None) -> list:
    """the wrapper on one frame: planes listed in `which` are processed with their slot's parameters (plane > 0 is chroma),
    the others are copies"""
    st, rs, rd = check_mosquito_args([planes[k].shape for k in which], strength, restore, radius)
    return [mosquito_nr(p, st[k], rs[k], rd[k], bits, k > 0) if k in which else p.copy() for k, p in enumerate(planes)]


# ---- the reference's golden cases (tests/goldens/mosquito.json), rebuilt from tests/fixtures.py ---------------------------

_FMT = {  # name -> (bits, ssw, ssh, float); Gray formats have no subsampling entry
    "GRAY8": (8, None, None, False), "GRAY10": (10, None, None, False), "GRAY12": (12, None, None, False), "GRAY14": (14, None, None, False),
    "GRAY16": (16, None, None, False), "GRAYS": (32, None, None, True), "YUV420P8": (8, 1, 1, False), "YUV420P16": (16, 1, 1, False),
    "YUV444P16": (16, 0, 0, False), "YUV444PS": (32, 0, 0, True),
}


def format_bits(fmt: str) -> int:
    return _FMT[fmt][0]


@lru_cache(maxsize=None)
def _planes(fmt: str, geometry: str) -> tuple:
    bits, ssw, ssh, flt = _FMT[fmt]
    if ssw is not None:
        assert geometry == "full"
        return tuple(fx.crop_yuv(bits, ssw, ssh, sample="f32") if flt else fx.crop_yuv(bits, ssw, ssh))
    if flt:
        p = fx.crop_grays()
    elif bits == 8:
        p = fx.crop_gray8()
    else:
        from oracle import vs_host as vh

        p = vh.rgb24_to_yuv(fx.crop_rgb24(), bits, gray=True)[0]
    p = _crop_gray(p, geometry)
    p.setflags(write=False)
    return (p,)


def golden_inputs(fmt: str, geometry: str) -> list:
    """the planes of a golden key's clip (frame 0)"""
    return list(_planes(fmt, geometry))


def parse_key(key: str):
    """'YUV444P16|full|planes=[1,2],strength=16' -> (fmt, geometry, keyword arguments of mosquito_frame): `which` from
    planes=[..] (default [0]), scalars or per-plane lists for strength / restore / radius"""
    fmt, geometry, args = key.split("|")
    kw, depth, item, items = {}, 0, "", []
    for ch in args + ",":
        if ch == "," and depth == 0:
            items.append(item)
            item = ""
            continue
        depth += (ch == "[") - (ch == "]")
        item += ch
    for it in items:
        k, v = it.split("=")
        val = [int(x) for x in v[1:-1].split(",")] if v.startswith("[") else int(v)
        kw["which" if k == "planes" else k] = tuple(val) if k == "planes" else val
    assert set(kw) <= {"which", "strength", "restore", "radius"}, key
    kw.setdefault("which", (0,))
    return fmt, geometry, kw


def run_key(key: str) -> list:
    """the spec's output planes for a golden key"""
    fmt, geometry, kw = parse_key(key)
    bits = format_bits(fmt)
    return mosquito_frame(golden_inputs(fmt, geometry), bits=None if bits == 32 else bits, **kw)


def golden_stats(p: np.ndarray, bits: int) -> dict:
    """fixtures.plane_stats with the average of an integer plane normalised by 2^bits - 1, as the reference's goldens are"""
    st = fx.plane_stats(p)
    if p.dtype.kind == "u":
        st["avg"] = float(p.astype(np.uint64).sum()) / p.size / float((1 << bits) - 1)
    return st


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "mosquito_goldens.json").read_text())
