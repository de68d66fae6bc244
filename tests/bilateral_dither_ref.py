"""Parity spec of vszip.BilateralDither (the port of dither's Dither_bilateral16) in numpy: what the create function of
src/vapoursynth/bilateral_dither.zig derives per plane (m, wmax, sum_w_min, dense or sub-sampled), the 23 point lists of
src/filters/bilateral_dither_subspl.zig (4-arm spirals for K < 32, a scan of a toroidal void-and-cluster matrix for K >= 32) and
what processPlane of src/filters/bilateral_dither.zig computes per sample, for 8..16-bit integer and 32-bit float planes, with
and without a `ref` plane that drives the weights.

Formulation. The reference pads a float cache by the radius with mirrored samples (edge duplicated) and addresses it linearly; every
tap (dx, dy) lies in [-(r-1), r-1]^2 and r <= w, r <= h, so each tap is the sample at (mirror(x + dx), mirror(y + dy)) with a single
reflection, which is what plane() gathers. The sub-sampled path reads four samples at base + offset for a group of four outputs: lane
e of the group is the same tap of output x + e. Every output is a fixed-order chain of f32 operations: per tap
wgt = max(min(m - |vr - cen_ref|, wmax), 0), sum_w += wgt, sum = fma(v - cen, wgt, sum); then cen + sum / max(sum_w, sum_w_min).

libm. The spiral lists use cos, sin and pow, the void-and-cluster kernel exp, all in f64 through Python's math module (the same libm
the C++ generator links).
"""
from __future__ import annotations

import json
import math
from functools import lru_cache

import numpy as np

import fixtures as fx

F = np.float32
M32 = 0xFFFFFFFF
NBR_POINT_LISTS = 23
MAX_SUBSPL_POINTS = 4096
SPIRAL_THRESHOLD = 32
VNC_KS = 9
DEFAULTS = dict(radius=16, thr=2.5, flat=0.4, wmin=0.0, subspl=0.0)
RANGES = dict(radius=(2, 16384), thr=(0, 65535), flat=(0, 1), wmin=(0, 65535), subspl=(0, 4096))


def _fmt(v) -> str:
    """Zig's {d}: integers without a point, f32 values in their shortest decimal form"""
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    v = F(v)
    return str(int(v)) if float(v) == int(v) and abs(float(v)) < 1e15 else str(v)


def check_range(key: str, v):
    lo, hi = RANGES[key]
    if v < lo:
        raise ValueError(f"BilateralDither: {key} value {_fmt(v)} is below minimum {_fmt(lo)}.")
    if v > hi:
        raise ValueError(f"BilateralDither: {key} value {_fmt(v)} is above maximum {_fmt(hi)}.")


# ---- create time ------------------------------------------------------------------------------------------------------------
def rint_f32(x: float) -> int:
    """fstb::round_int of a value cast to f32: nearbyintf, ties to even"""
    return int(round(float(F(x))))


def points_k(radius: int, subspl) -> int:
    area = (2 * radius - 1) ** 2
    s = float(F(subspl))
    actual = float(2 * radius) if s < 1e-3 else s
    return min(max(rint_f32(area / actual), 3), MAX_SUBSPL_POINTS)


def derive(is_float: bool, bits: int, radius: int, thr=2.5, flat=0.4, wmin=0.0, subspl=0.0) -> dict:
    """per plane: m, wmax, sum_w_min (f32), K (0 for the dense path), subsampled, peak"""
    radius = int(radius)
    check_range("radius", radius)
    thr, flat, wmin, subspl = F(thr), F(flat), F(wmin), F(subspl)
    for k, v in (("thr", thr), ("flat", flat), ("wmin", wmin), ("subspl", subspl)):
        check_range(k, v)
    scale = F(1.0 / 256.0) if is_float else F(1 << (bits - 8))
    unit = F(1.0) / F(65535.0) if is_float else F(1.0)
    m = max(F(thr * scale), unit)
    wmax = max(F(F(thr * F(F(1.0) - flat)) * scale), unit)
    sub = bool(subspl >= F(4.0)) or float(subspl) < 1e-3
    k = points_k(radius, subspl) if sub else 0
    n = F(k) if sub else F((2 * radius - 1) * (2 * radius - 1))
    swmin = max(F(F(wmin * wmax) * n), unit)
    return dict(m=F(m), wmax=F(wmax), sum_w_min=F(swmin), K=k, subsampled=sub, peak=F(0.0 if is_float else (1 << bits) - 1))


def lcg(v: int) -> int:
    return (v * 1664525 + 1013904223) & M32


def row_starts(h: int) -> np.ndarray:
    """start(y) = (LCG^(y+1)(1) >> 8) % 23"""
    out, v = np.empty(h, np.int64), 1
    for y in range(h):
        v = lcg(v)
        out[y] = (v >> 8) % NBR_POINT_LISTS
    return out


class _Minstd:
    """libstdc++'s minstd_rand0 with uniform_int_distribution<int>(0, n - 1)"""

    def __init__(self, seed=1):
        s = seed % 2147483647
        self.s = s if s else 1

    def dist(self, n: int) -> int:
        scaling = 2147483645 // n
        past = n * scaling
        while True:
            self.s = (self.s * 16807) % 2147483647
            ret = self.s - 1
            if ret < past:
                return ret // scaling


def _vnc_kernel() -> np.ndarray:
    """kern[j + 4, i + 4] = exp(-(i^2 + j^2) / (2 * 1.5^2))"""
    inv2s2 = 1.0 / (2.0 * 1.5 * 1.5)
    k = np.empty((VNC_KS, VNC_KS), np.float64)
    for j in range(-4, 5):
        for i in range(-4, 5):
            k[j + 4, i + 4] = math.exp(-float(i * i + j * j) * inv2s2)
    return k


def _find_cluster(mat: np.ndarray, kern: np.ndarray, color: int):
    """the first cell (scan order) of `color` whose Gaussian sum over the toroidal 9 x 9 neighbourhood of the same colour is the largest:
    81 rolled masked adds in the reference's (j, i) order; adding 0.0 for a cell of the other colour equals skipping it"""
    mask = (mat == color).astype(np.float64)
    s = np.zeros(mat.shape, np.float64)
    for j in range(-4, 5):
        rj = np.roll(mask, -j, axis=0)
        for i in range(-4, 5):
            s = s + np.roll(rj, -i, axis=1) * kern[j + 4, i + 4]
    s = np.where(mat == color, s, -np.inf)
    at = int(np.argmax(s))
    if s.flat[at] == -np.inf:
        return 0, 0
    return at % mat.shape[1], at // mat.shape[1]


@lru_cache(maxsize=None)
def vnc_matrix(n: int) -> np.ndarray:
    """createVncMatrix: [y, x] -> rank 0 .. n*n - 1; depends on the size alone"""
    kern = _vnc_kernel()
    base = np.zeros((n, n), np.uint16)
    err = np.zeros((n, n), np.float64)
    d = 1
    for _ in range(2):
        for y in range(n):
            xs = range(n - 1, -1, -1) if d < 0 else range(n)
            for x in xs:
                val = 0.1 + err[y, x]
                err[y, x] = 0.0
                q = min(max(rint_f32(val), 0), 1)
                base[y, x] = q
                e = val - float(q)
                err[y, (x + d) % n] += e * 0.5
                err[(y + 1) % n, (x - d) % n] += e * 0.25
                err[(y + 1) % n, x] += e * 0.25
            d = -d
    while True:
        cx, cy = _find_cluster(base, kern, 1)
        base[cy, cx] = 0
        vx, vy = _find_cluster(base, kern, 0)
        base[vy, vx] = 1
        if (cx, cy) == (vx, vy):
            break
    vnc = np.zeros((n, n), np.int64)
    ones = int((base == 1).sum())
    mat, rank = base.copy(), ones
    while rank > 0:
        rank -= 1
        x, y = _find_cluster(mat, kern, 1)
        mat[y, x] = 0
        vnc[y, x] = rank
    mat, rank = base.copy(), ones
    while rank < n * n:
        x, y = _find_cluster(mat, kern, 0)
        mat[y, x] = 1
        vnc[y, x] = rank
        rank += 1
    vnc.setflags(write=False)
    return vnc


@lru_cache(maxsize=None)
def point_lists(radius: int, subspl) -> np.ndarray:
    """generate(r, r, subspl): (23, K, 2) int16, [..., 0] = x, [..., 1] = y"""
    r = int(radius)
    s = float(F(subspl))
    actual = float(2 * r) if s < 1e-3 else s
    K = points_k(r, subspl)
    win = 2 * r - 1
    n = min(max(win * 3 // 2, 16), 32)
    pts = np.zeros((NBR_POINT_LISTS, K, 2), np.int16)
    ms_a, ms_x, ms_y = _Minstd(1), _Minstd(1), _Minstd(1)
    rnd = 1
    for lc in range(NBR_POINT_LISTS):
        done = np.zeros(win * win, bool)
        done[(r - 1) + (r - 1) * win] = True
        cnt = 1
        if K < SPIRAL_THRESHOLD:
            angle_base = float(ms_a.dist(NBR_POINT_LISTS)) * (math.pi * 0.5 / float(NBR_POINT_LISTS))
            arm_dir = 1 - (lc & 2)
            narm = 4
            npa = (K - 1) // narm
            amul = 2.0 * math.pi / float(narm) * float(arm_dir)
            for p in range(npa):
                posd = math.pow(float(p) / float(npa), 3.0 / 5.0)
                for a in range(narm):
                    ang = angle_base + (posd * 2.0 + float(a)) * amul
                    x = rint_f32(math.cos(ang) * posd * float(r - 1))
                    y = rint_f32(math.sin(ang) * posd * float(r - 1))
                    da = (x + r - 1) + (y + r - 1) * win
                    if 0 <= da < win * win and not done[da]:
                        pts[lc, cnt] = (x, y)
                        done[da] = True
                        cnt += 1
            while cnt < K:
                rnd = lcg(rnd)
                x = ((rnd >> 8) % win) - (r - 1)
                rnd = lcg(rnd)
                y = ((rnd >> 8) % win) - (r - 1)
                da = (x + r - 1) + (y + r - 1) * win
                if not done[da]:
                    pts[lc, cnt] = (x, y)
                    done[da] = True
                    cnt += 1
        else:
            vnc = vnc_matrix(n)
            ofs_x, ofs_y = ms_x.dist(win), ms_y.dist(win)
            trg = int(math.floor(float(n * n) / actual))
            yy, xx = np.mgrid[0:win, 0:win]
            v = vnc[(yy + ofs_y) % n, (xx + ofs_x) % n]
            # the scan takes levels [0, trg), then one level a pass: a cell of rank v is met in pass max(v - trg + 1, 0), in (y, x) order
            order = np.argsort((np.maximum(v - trg + 1, 0) * (win * win) + yy * win + xx).ravel(), kind="stable")
            order = order[order != (r - 1) + (r - 1) * win][:K - 1]
            pts[lc, 1:, 0] = order % win - (r - 1)
            pts[lc, 1:, 1] = order // win - (r - 1)
    pts.setflags(write=False)
    return pts


def checksum(pts: np.ndarray) -> int:
    """position-sensitive sum of the 16-bit patterns, modulo 2^64 (what tests/bilateral_dither_points_check.cpp prints)"""
    u = np.ascontiguousarray(pts).view(np.uint16).ravel().astype(np.uint64)
    i = np.arange(u.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(((u + np.uint64(1)) * (i * np.uint64(2654435761) + np.uint64(12345))).sum(dtype=np.uint64))


# ---- the filter -------------------------------------------------------------------------------------------------------------
def _mirror(i: np.ndarray, n: int) -> np.ndarray:
    i = np.where(i < 0, -1 - i, i)
    return np.where(i >= n, 2 * n - 1 - i, i)


def weights(vr, cen_ref, m, wmax):
    return np.maximum(np.minimum(F(m) - np.abs(vr - cen_ref), F(wmax)), F(0.0)).astype(F)


def accumulate(src, radius, m, wmax, pts=None, ref=None, classes=None):
    """-> cen, sum, sum_w (f32 planes) after every tap in order. classes: a list that receives the counts of taps with weight zero,
    saturated at wmax and in between (branch coverage)."""
    from oracle.vs_host import fma32

    h, w = src.shape
    r = int(radius)
    if w < r or h < r:
        raise ValueError('BilateralDither: picture size must be greater than "radius"')
    p = r - 1
    ys, xs = _mirror(np.arange(-p, h + p), h), _mirror(np.arange(-p, w + p), w)
    S = src.astype(F)[ys][:, xs]
    R = S if ref is None else ref.astype(F)[ys][:, xs]
    cen, cen_ref = S[p:p + h, p:p + w], R[p:p + h, p:p + w]
    acc, acc_w = np.zeros((h, w), F), np.zeros((h, w), F)
    cls = np.zeros(3, np.int64)

    def tap(v, vr):
        nonlocal acc, acc_w
        wgt = weights(vr, cen_ref, m, wmax)
        acc_w = (acc_w + wgt).astype(F)
        acc = fma32((v - cen).astype(F), wgt, acc)
        if classes is not None:
            cls[0] += int((wgt == 0).sum())
            cls[1] += int((wgt == F(wmax)).sum())
            cls[2] += int(((wgt > 0) & (wgt < F(wmax))).sum())
    if pts is None:
        for dy in range(-p, p + 1):
            for dx in range(-p, p + 1):
                tap(S[p + dy:p + dy + h, p + dx:p + dx + w], R[p + dy:p + dy + h, p + dx:p + dx + w])
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        lst = (row_starts(h)[:, None] + (xx >> 2)) % NBR_POINT_LISTS
        for k in range(pts.shape[1]):
            gy, gx = yy + p + pts[lst, k, 1], xx + p + pts[lst, k, 0]
            tap(S[gy, gx], R[gy, gx])
    if classes is not None:
        classes.append(cls)
    return cen, acc, acc_w


def plane(src, radius, m, wmax, sum_w_min, bits=0, pts=None, ref=None) -> np.ndarray:
    """processPlane: src (u8 | u16 | f32); pts None: the dense window; bits: the sample depth of integer planes"""
    cen, acc, acc_w = accumulate(src, radius, m, wmax, pts, ref)
    out = (cen + (acc / np.maximum(acc_w, F(sum_w_min))).astype(F)).astype(F)
    if src.dtype == np.float32:
        return out
    q = np.clip(out, F(0.0), F((1 << bits) - 1)).astype(np.float64)
    return np.floor(q + 0.5).astype(src.dtype)  # (round half away from zero of a value >= 0; exact in f64)


def filter_plane(src, bits=None, ref=None, **kw) -> np.ndarray:
    """one plane through derive(), point_lists() and plane()"""
    f = src.dtype == np.float32
    bits = 32 if f else (bits or 8 * src.dtype.itemsize)
    a = dict(DEFAULTS, **kw)
    d = derive(f, bits, a["radius"], a["thr"], a["flat"], a["wmin"], a["subspl"])
    pts = point_lists(int(a["radius"]), float(F(a["subspl"]))) if d["subsampled"] else None
    return plane(src, a["radius"], d["m"], d["wmax"], d["sum_w_min"], bits, pts, ref)


def _array(key, v):
    a = [DEFAULTS[key]] if v is None else ([v] if np.isscalar(v) else list(v))
    if len(a) > 3:
        raise ValueError(f"BilateralDither: {key} has too many elements (got {len(a)}, max 3).")
    return [a[min(i, len(a) - 1)] for i in range(3)]


def frame(planes_in, bits=None, ssw=0, ssh=0, ref=None, planes=None, radius=None, thr=None, flat=None, wmin=None, subspl=None) -> list:
    """vszip.BilateralDither on one frame: per-plane arrays of up to three values (the last repeats); planes not selected are copies"""
    arr = {k: _array(k, v) for k, v in (("radius", radius), ("thr", thr), ("flat", flat), ("wmin", wmin), ("subspl", subspl))}
    for k in ("radius", "thr", "flat", "wmin", "subspl"):
        for i in range(3):
            check_range(k, arr[k][i] if k == "radius" else F(arr[k][i]))
    h, w = planes_in[0].shape
    if w < 16 or h < 16:
        raise ValueError("BilateralDither: input must be 16x16 min")
    sel = list(range(len(planes_in))) if planes is None else list(planes)
    out = []
    for i, p in enumerate(planes_in):
        if i not in sel:
            out.append(p.copy())
            continue
        out.append(filter_plane(p, bits, None if ref is None else ref[i], **{k: arr[k][i] for k in arr}))
    return out


# ---- the reference's golden cases (tests/goldens/bilateral_dither.json), rebuilt from tests/fixtures.py ----------------------------
_FMT = {  # name -> (family, bits, ssw, ssh, float)
    "GRAY8": ("GRAY", 8, 0, 0, False), "GRAY16": ("GRAY", 16, 0, 0, False), "GRAYS": ("GRAY", 32, 0, 0, True), "YUV420P8": ("YUV", 8, 1, 1, False),
    "YUV420P16": ("YUV", 16, 1, 1, False), "YUV444P16": ("YUV", 16, 0, 0, False), "YUV444PS": ("YUV", 32, 0, 0, True), "RGB24": ("RGB", 8, 0, 0, False),
    "RGBS": ("RGB", 32, 0, 0, True),
}


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "bilateral_dither_goldens.json").read_text())


def parse_key(key: str):
    """'YUV420P8|full|radius=[8,4,4],subspl=2,thr=[8,12,12]' -> (format, geometry, keyword arguments)"""
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
    return fmt, geometry, kw


@lru_cache(maxsize=None)
def _planes(fmt: str, geometry: str) -> tuple:
    family, bits, ssw, ssh, flt = _FMT[fmt]
    if family == "YUV":
        p = fx.yuv_geometry(fx.crop_yuv(bits, ssw, ssh, sample="f32") if flt else fx.crop_yuv(bits, ssw, ssh), geometry, ssw, ssh)
    elif family == "RGB":
        assert geometry == "full"
        p = [np.ascontiguousarray(c) for c in (fx.crop_rgbs() if flt else fx.crop_rgb24())]
    else:
        g = fx.crop_grays() if flt else (fx.crop_gray8() if bits == 8 else fx.crop_gray16())
        assert geometry in ("full", "odd")
        p = [np.ascontiguousarray(g if geometry == "full" else g[:-1, :-1])]
    for x in p:
        x.setflags(write=False)
    return tuple(p)


def golden_inputs(fmt: str, geometry: str) -> list:
    return list(_planes(fmt, geometry))


def run_key(key: str) -> list:
    fmt, geometry, kw = parse_key(key)
    family, bits, ssw, ssh, flt = _FMT[fmt]
    return frame(golden_inputs(fmt, geometry), bits, ssw, ssh, **kw)


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def noisy_plane(seed: int, h: int, w: int, dtype) -> np.ndarray:
    """natural content at half scale with noise of an eighth (u8 / u16: tiled_natural // 2 + (splitmix64 >> 4); f32: * 0.5 + noise * 0.06):
    with thr = 8 every weight class and the sum_w_min floor take part (tests/test_bilateral_dither_ref.py counts them)"""
    a, n = fx.tiled_natural((h, w), dtype, seed % 3), fx.splitmix64_plane(seed, (h, w), dtype)
    if np.dtype(dtype) == np.float32:
        p = (a * F(0.5) + n * F(0.06)).astype(F)
    else:
        p = (a // 2 + (n >> 4)).astype(dtype)
    p.setflags(write=False)
    return p
