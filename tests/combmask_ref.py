"""CPU parity spec of CombMask and CombMaskMT (the reference's src/filters/comb_mask.zig and comb_mask_mt.zig with the
create-time rules of src/vapoursynth/comb_mask.zig / comb_mask_mt.zig): a numpy restatement that reproduces every key of
the reference's tests/goldens/combmask.json from tests/fixtures.py's inputs (tests/test_combmask_ref.py).
tests/test_gpu_combmask.py checks vszip_comb_mask / vszip_comb_mask_mt against it bit for bit.

Only [0, w) x h of a plane is an input or an output here (include/vszip_hip.h, "Plane memory"); the reference's vector
loops also touch the pitch padding.

Not part of oracle/ (frozen): a test-support module like fixtures.py.
"""
from __future__ import annotations

import json
from functools import lru_cache

import numpy as np

import fixtures as fx


def _mirror_rows(h: int, off: int) -> np.ndarray:
    """row y + off, mirrored without repeating the edge row (-1 -> 1, h -> h - 2)"""
    y = np.arange(h) + off
    y = np.where(y < 0, -y, y)
    return np.where(y >= h, 2 * (h - 1) - y, y)


def check_comb_mask_args(heights, cthresh: int, mthresh: int, metric: int):
    """combMaskCreate's checks, in its order; ValueError with its wording"""
    cth_max = 65025 if metric else 255
    if cthresh > cth_max or cthresh < 0:
        raise ValueError(f"CombMask: cthresh must be between 0 and {cth_max} when metric = {'true' if metric else 'false'}.")
    if mthresh > 255 or mthresh < 0:
        raise ValueError("CombMask: mthresh must be between 0 and 255.")
    if min(heights) < 3:
        raise ValueError("CombMask: clip too small; every plane must be at least 3 rows tall.")


def comb_mask(src: np.ndarray, prv: np.ndarray | None = None, cthresh: int = 6, mthresh: int = 9, expand: bool = True, metric: int = 0) -> np.ndarray:
    """one 2-D uint8 plane of frame n; prv: the same plane of frame max(0, n - 1) (needed when mthresh > 0)"""
    assert src.dtype == np.uint8 and src.ndim == 2
    h, w = src.shape
    check_comb_mask_args([h], cthresh, mthresh, metric)
    s = src.astype(np.int32)
    b, c, d = s[_mirror_rows(h, -1)], s, s[_mirror_rows(h, 1)]
    if metric:
        m = (b - c) * (d - c) > cthresh
    else:
        a, e = s[_mirror_rows(h, -2)], s[_mirror_rows(h, 2)]
        d1, d2 = c - b, c - d
        m = ((d1 > cthresh) & (d2 > cthresh)) | ((d1 < -cthresh) & (d2 < -cthresh))
        m &= np.abs(a + 4 * c + e - 3 * (b + d)) > 6 * cthresh
    if mthresh > 0:
        assert prv is not None and prv.shape == src.shape and prv.dtype == np.uint8
        mo = np.abs(s - prv.astype(np.int32)) > mthresh
        dil = mo.copy()
        dil[1:] |= mo[:-1]  # nothing above row 0
        dil[:-1] |= mo[1:]  # below row h - 1: that row itself
        m &= dil
    if expand and w >= 2:
        x = m.copy()
        x[:, 0] = m[:, 0] | m[:, 1]
        x[:, 1:w - 1] = m[:, 0:w - 2] | m[:, 1:w - 1] | m[:, 2:w]
        m = x  # column w - 1 keeps its unexpanded value
    return np.where(m, 255, 0).astype(np.uint8)


def check_comb_mask_mt_args(heights, thy1: int, thy2: int):
    if thy1 > 255 or thy1 < 0:
        raise ValueError("CombMaskMT: thY1 value should be in range [0;255]")
    if thy2 > 255 or thy2 < 0:
        raise ValueError("CombMaskMT: thY2 value should be in range [0;255]")
    if thy1 > thy2:
        raise ValueError("CombMaskMT: thY1 can't be greater than thY2")
    if min(heights) < 3:
        raise ValueError("CombMaskMT: clip too small; every plane must be at least 3 rows tall.")


def comb_mask_mt(src: np.ndarray, thy1: int = 30, thy2: int = 30) -> np.ndarray:
    assert src.dtype == np.uint8 and src.ndim == 2
    h, w = src.shape
    check_comb_mask_mt_args([h], thy1, thy2)
    s = src.astype(np.int32)
    p = (s[:-2] - s[1:-1]) * (s[2:] - s[1:-1])
    out = np.zeros((h, w), np.uint8)
    if thy1 == thy2:
        out[1:-1] = np.where(p > thy2, 255, 0)
    else:
        gray = np.minimum(np.maximum(p - thy1, 0) * 256 // (thy2 - thy1), 255)  # selected only where p >= thY1: floor == truncation
        out[1:-1] = np.where(p < thy1, 0, np.where(p > thy2, 255, gray))
    return out


# ---- the reference's golden cases (tests/goldens/combmask.json), rebuilt from tests/fixtures.py ------------------------

_SS = {"YUV420P8": (1, 1), "YUV444P8": (0, 0)}


def _crop_gray(p: np.ndarray, geometry: str) -> np.ndarray:
    """reference tests/conftest.py _geometry on a Gray clip"""
    if geometry == "full":
        return np.ascontiguousarray(p)
    if geometry == "odd":
        return np.ascontiguousarray(p[:-1, :-1])
    if geometry == "tiny":
        return np.ascontiguousarray(p[100:107, 200:213])
    raise ValueError(geometry)


def temporal_planes(fmt: str, geometry: str, n: int) -> list:
    """frame n of the reference's make_temporal_clip(fmt, geometry): the shifted crop through a POINT resize"""
    if fmt == "GRAY8":
        return [_crop_gray(fx.luma8(fx.temporal_rgb24(n)), geometry)]
    from oracle import vs_host as vh

    ssw, ssh = _SS[fmt]
    return fx.yuv_geometry(vh.rgb24_to_yuv(fx.temporal_rgb24(n), 8, ssw, ssh, kind="point"), geometry, ssw, ssh)


def golden_inputs(fmt: str, geometry: str, filt: str):
    """-> (source planes, previous frame's planes or None) of a golden key's clip: CombMask is read at frame 1 of the
    temporal clip, CombMaskMT at frame 0 of the still one (bilinear YUV)"""
    if filt == "CombMask":
        return temporal_planes(fmt, geometry, 1), temporal_planes(fmt, geometry, 0)
    if fmt == "GRAY8":
        return [_crop_gray(fx.crop_gray8(), geometry)], None
    ssw, ssh = _SS[fmt]
    return fx.yuv_geometry(fx.crop_yuv(8, ssw, ssh), geometry, ssw, ssh), None


def parse_key(key: str):
    """'GRAY8|full|cthresh=8,expand=0,mthresh=50|CombMask' -> (fmt, geometry, filter, keyword arguments of comb_mask / comb_mask_mt)"""
    fmt, geometry, args, filt = key.split("|")
    assert filt in ("CombMask", "CombMaskMT"), key
    kw = {}
    if args != "default":
        for item in args.split(","):
            k, v = item.split("=")
            kw[k] = int(v)
    if filt == "CombMask":
        assert set(kw) <= {"cthresh", "mthresh", "expand", "metric"}, key
        if "expand" in kw:
            kw["expand"] = bool(kw["expand"])
    else:
        assert set(kw) <= {"thY1", "thY2"}, key
        kw = {k.lower(): v for k, v in kw.items()}
    return fmt, geometry, filt, kw


def run_key(key: str) -> list:
    """the spec's output planes for a golden key"""
    fmt, geometry, filt, kw = parse_key(key)
    srcs, prvs = golden_inputs(fmt, geometry, filt)
    if filt == "CombMask":
        return [comb_mask(s, p, **kw) for s, p in zip(srcs, prvs)]
    return [comb_mask_mt(s, **kw) for s in srcs]


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "combmask_goldens.json").read_text())
