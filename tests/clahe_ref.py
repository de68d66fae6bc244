"""CPU parity spec of CLAHE (the reference's filter.applyCLAHE, src/filters/clahe.zig:14-282): a numpy restatement
that reproduces every key of the reference's tests/goldens/clahe.json from tests/fixtures.py's inputs
(tests/test_clahe_ref.py). tests/test_gpu_clahe.py checks vszip_clahe against it bit for bit.

Not part of oracle/ (frozen): a test-support module like fixtures.py.
"""
from __future__ import annotations

import json
import re
from functools import lru_cache

import numpy as np

import fixtures as fx

f32 = np.float32
INT32_MAX = (1 << 31) - 1


def clip_limit(w: int, h: int, limit: int, tiles, hist_size: int) -> int:
    """clahe.zig:32-33 (u64 product, truncated; at least 1)"""
    tw, th = w // tiles[0], h // tiles[1]
    return max(limit * tw * th // hist_size, 1)


def luts(src: np.ndarray, limit: int, tiles) -> np.ndarray:
    """calcLut (clahe.zig:40-156): [tiles_y][tiles_x][hist_size] of the sample type"""
    h, w = src.shape
    hs = 256 if src.dtype == np.uint8 else 65536
    tx_n, ty_n = tiles
    tw, th = w // tx_n, h // ty_n
    tot = tw * th
    scale = f32(f32(hs - 1) / f32(tot))
    cl = clip_limit(w, h, limit, tiles, hs)
    lut = np.zeros((ty_n, tx_n, hs), src.dtype)
    for ty in range(ty_n):
        for tx in range(tx_n):
            hist = np.bincount(src[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=hs).astype(np.int64)
            clipped = int(np.maximum(hist - cl, 0).sum())
            hist = np.minimum(hist, cl)
            rb = clipped // hs
            res = clipped - rb * hs
            hist += rb
            if res:
                step = max(hs // res, 1)
                i = 0
                while i < hs and res > 0:
                    hist[i] += 1
                    res -= 1
                    i += step
            lut[ty, tx] = np.trunc(np.cumsum(hist).astype(f32) * scale + f32(0.5)).astype(src.dtype)
    return lut


def clahe(src: np.ndarray, limit: int = 7, tiles=(3, 3)) -> np.ndarray:
    """applyCLAHE on one 2-D uint8 / uint16 plane; tiles = (tiles_x, tiles_y)"""
    h, w = src.shape
    tx_n, ty_n = tiles
    tw, th = w // tx_n, h // ty_n
    lut = luts(src, limit, tiles)
    txf = np.arange(w, dtype=f32) * (f32(1) / f32(tw)) - f32(0.5)
    tx1 = np.floor(txf).astype(np.int64)
    xa = (txf - tx1.astype(f32)).astype(f32)
    tx2 = np.minimum(tx1 + 1, tx_n - 1)
    tx1 = np.clip(tx1, 0, tx_n - 1)
    out = np.empty_like(src)
    omx = (f32(1) - xa).astype(f32)
    for y in range(h):
        tyf = f32(f32(y) * (f32(1) / f32(th)) - f32(0.5))
        t1 = int(np.floor(tyf))
        ya = f32(tyf - f32(t1))
        t2 = min(t1 + 1, ty_n - 1)
        t1 = min(max(t1, 0), ty_n - 1)
        s = src[y]
        l0, l1 = lut[t1, tx1, s].astype(f32), lut[t1, tx2, s].astype(f32)
        l2, l3 = lut[t2, tx1, s].astype(f32), lut[t2, tx2, s].astype(f32)
        out[y] = np.trunc((l0 * omx + l1 * xa) * f32(f32(1) - ya) + (l2 * omx + l3 * xa) * ya + f32(0.5)).astype(src.dtype)
    return out


def parse_tiles(tiles) -> tuple:
    """the wrapper's `tiles` argument (clahe.zig(vs):76-91): an int, [n] or [x, y]"""
    if isinstance(tiles, (int, np.integer)):
        tiles = [int(tiles)]
    tiles = [int(t) for t in tiles]
    if len(tiles) < 1 or len(tiles) > 2:
        raise ValueError("CLAHE : tiles array can't have more than 2 values.")
    return (tiles[0], tiles[1] if len(tiles) == 2 else tiles[0])


# ---- the reference's golden cases (tests/goldens/clahe.json), rebuilt from tests/fixtures.py ----------------------------

_SS = {"YUV420P8": (8, 1, 1), "YUV444P8": (8, 0, 0), "YUV420P16": (16, 1, 1), "YUV444P16": (16, 0, 0)}


def _crop_geometry(planes, geometry: str) -> list:
    """reference tests/conftest.py _geometry on an unsubsampled clip (Gray, RGB)"""
    if geometry == "full":
        return [np.ascontiguousarray(p) for p in planes]
    if geometry == "odd":
        return [np.ascontiguousarray(p[:-1, :-1]) for p in planes]
    if geometry == "tiny":
        return [np.ascontiguousarray(p[100:107, 200:213]) for p in planes]
    raise ValueError(geometry)


def golden_inputs(fmt: str, geometry: str) -> list:
    """the source planes of a golden key's clip"""
    if fmt == "GRAY8":
        return _crop_geometry([fx.crop_gray8()], geometry)
    if fmt == "GRAY16":
        return _crop_geometry([fx.crop_gray16()], geometry)
    if fmt == "RGB24":
        return _crop_geometry(list(fx.crop_rgb24()), geometry)
    if fmt == "RGB48":
        return _crop_geometry([p.astype(np.uint16) * np.uint16(257) for p in fx.crop_rgb24()], geometry)
    bits, ssw, ssh = _SS[fmt]
    return fx.yuv_geometry(fx.crop_yuv(bits, ssw, ssh), geometry, ssw, ssh)


def parse_key(key: str):
    """'YUV420P16|full|limit=1024,tiles=[8,2]' -> (fmt, geometry, limit, (tiles_x, tiles_y))"""
    fmt, geometry, args = key.split("|")[:3]
    m = re.fullmatch(r"limit=(\d+),tiles=(\d+|\[\d+,\d+\])", args)
    assert m, key
    t = json.loads(m.group(2))
    return fmt, geometry, int(m.group(1)), parse_tiles(t)


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "clahe_goldens.json").read_text())
