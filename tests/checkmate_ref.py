"""CPU parity spec of Checkmate (the reference's src/filters/checkmate.zig with the create-time rules and the frame
requests of src/vapoursynth/checkmate.zig): a numpy restatement that reproduces every key of the reference's
tests/goldens/checkmate.json from tests/fixtures.py's inputs (tests/test_checkmate_ref.py).
tests/test_gpu_checkmate.py checks vszip_checkmate against it bit for bit.

Only [0, w) x h of a plane is an input or an output here (include/vszip_hip.h, "Plane memory"); the reference's copy of
the two edge rows at either end also moves the pitch padding.

Not part of oracle/ (frozen): a test-support module like fixtures.py.
"""
from __future__ import annotations

import json
from functools import lru_cache

import numpy as np

import fixtures as fx
from combmask_ref import _crop_gray


def check_checkmate_args(sizes, thr: int, tmax: int, tthr2: int):
    """checkmateCreate's checks, in its order; ValueError with its wording. sizes: (h, w) of every plane"""
    if tmax < 1 or tmax > 255:
        raise ValueError("Checkmate: tmax value should be in range [1;255].")
    if tthr2 < 0:
        raise ValueError("Checkmate: tthr2 should be non-negative.")
    if thr < 0 or thr > 255:
        raise ValueError("Checkmate: thr value should be in range [0;255].")
    if any(w < 3 or h < 5 for h, w in sizes):
        raise ValueError("Checkmate: clip too small; every plane must be at least 3 wide and 5 tall.")


def intermediates(p1, cur, n1, thr: int = 12, tmax: int = 12) -> dict:
    """the spatial form's per-sample values on rows 2 .. h - 3 (int64 arrays of (h - 4) x w): curr, the weights, and the
    output before saturation"""
    h, w = cur.shape
    c, p, n = (a.astype(np.int64) for a in (cur, p1, n1))
    up, mid, dn = slice(0, h - 4), slice(2, h - 2), slice(4, h)  # rows y - 2, y, y + 2
    x = np.arange(w)
    xl, xr = np.maximum(x - 2, 0), np.minimum(x + 2, w - 1)  # clamped, not mirrored
    col = lambda f: f[up] + 2 * f[mid] + f[dn]
    cc = col(c)
    curr = -c[up][:, xl] - c[up][:, xr] + 2 * c[mid][:, xl] + 2 * c[mid][:, xr] - c[dn][:, xl] - c[dn][:, xr] + 2 * cc + 12 * c[mid]
    mult = 8192 // tmax
    weight = lambda f: np.minimum(np.clip(thr + tmax - np.abs(col(f) - cc), 0, tmax + 1) * mult, 8192)
    nw, pw = weight(n), weight(p)
    cw = 16384 - nw - pw
    q = np.sign(curr) * (np.abs(curr) // 10)  # the division truncates toward zero
    out = (cw * q + pw * (c[mid] + p[mid]) + nw * (c[mid] + n[mid])) >> 15  # arithmetic shift
    return {"curr": curr, "nw": nw, "pw": pw, "cw": cw, "out": out}


def checkmate(p2, p1, cur, n1, n2, thr: int = 12, tmax: int = 12, tthr2: int = 0) -> np.ndarray:
    """one 2-D uint8 plane of frame n; p2, p1, n1, n2: the same plane of frames n - 2 .. n + 2, clamped to the clip by the
    caller (p2 and n2 may be None when tthr2 == 0)"""
    assert cur.dtype == np.uint8 and cur.ndim == 2
    h, w = cur.shape
    check_checkmate_args([(h, w)], thr, tmax, tthr2)
    assert p1.shape == n1.shape == cur.shape and p1.dtype == n1.dtype == np.uint8
    out = cur.copy()  # rows 0, 1, h - 2, h - 1
    mid = slice(2, h - 2)
    res = np.clip(intermediates(p1, cur, n1, thr, tmax)["out"], 0, 255)
    if tthr2 > 0:
        assert p2 is not None and n2 is not None and p2.shape == n2.shape == cur.shape
        c, a, b, a2, b2 = (f[mid].astype(np.int64) for f in (cur, p1, n1, p2, n2))
        blend = (np.abs(a - b) < tthr2) & (np.abs(a2 - c) < tthr2) & (np.abs(c - b2) < tthr2)
        res = np.where(blend, (a + 2 * c + b) >> 2, res)
    out[mid] = res.astype(np.uint8)
    return out


def blend_mask(p2, p1, cur, n1, n2, tthr2: int) -> np.ndarray:
    """rows 2 .. h - 3: where the temporal branch is taken"""
    c, a, b, a2, b2 = (f[2:-2].astype(np.int64) for f in (cur, p1, n1, p2, n2))
    return (np.abs(a - b) < tthr2) & (np.abs(a2 - c) < tthr2) & (np.abs(c - b2) < tthr2)


def neighbour_indices(n: int, nframes: int):
    """(p2, p1, n1, n2) of frame n, as getFrame requests them"""
    return max(0, n - 2), max(0, n - 1), min(n + 1, nframes - 1), min(n + 2, nframes - 1)


def checkmate_clip(frames, thr: int = 12, tmax: int = 12, tthr2: int = 0) -> list:
    """every frame of a clip; frames[f]: a plane, or a list of planes -> the same structure"""
    out = []
    for n, f in enumerate(frames):
        i2, i1, j1, j2 = neighbour_indices(n, len(frames))
        if isinstance(f, np.ndarray):
            out.append(checkmate(frames[i2], frames[i1], f, frames[j1], frames[j2], thr, tmax, tthr2))
        else:
            out.append([checkmate(frames[i2][k], frames[i1][k], f[k], frames[j1][k], frames[j2][k], thr, tmax, tthr2) for k in range(len(f))])
    return out


# ---- the reference's golden cases (tests/goldens/checkmate.json), rebuilt from tests/fixtures.py ------------------------

_SS = {"YUV420P8": (1, 1), "YUV422P8": (1, 0), "YUV444P8": (0, 0)}


@lru_cache(maxsize=None)
def _temporal_planes(fmt: str, geometry: str, n: int) -> tuple:
    """frame n of the reference's make_temporal_clip(fmt, geometry)"""
    if fmt == "GRAY8":
        return (_crop_gray(fx.luma8(fx.temporal_rgb24(n)), geometry),)
    if fmt == "RGB24":
        assert geometry == "full"
        return tuple(np.ascontiguousarray(p) for p in fx.temporal_rgb24(n))
    from oracle import vs_host as vh

    ssw, ssh = _SS[fmt]
    return tuple(fx.yuv_geometry(vh.rgb24_to_yuv(fx.temporal_rgb24(n), 8, ssw, ssh, kind="point"), geometry, ssw, ssh))


def golden_inputs(fmt: str, geometry: str):
    """-> [frame 0, frame 1, frame 2] (lists of planes) of a golden key's 3-frame clip; every key is read at frame 1"""
    return [list(_temporal_planes(fmt, geometry, n)) for n in range(3)]


def parse_key(key: str):
    """'GRAY8|full|thr=12,tmax=12,tthr2=4' -> (fmt, geometry, keyword arguments of checkmate)"""
    fmt, geometry, args = key.split("|")
    kw = {}
    for item in args.split(","):
        k, v = item.split("=")
        kw[k] = int(v)
    assert set(kw) <= {"thr", "tmax", "tthr2"}, key
    return fmt, geometry, kw


def run_key(key: str) -> list:
    """the spec's output planes for a golden key"""
    fmt, geometry, kw = parse_key(key)
    clip = golden_inputs(fmt, geometry)
    return checkmate_clip(clip, **kw)[1]


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "checkmate_goldens.json").read_text())
