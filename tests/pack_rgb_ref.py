"""vszip.PackRGB in numpy: the spec the device is compared with (tests/test_gpu_pack_rgb*.py), and the inputs of the reference's six
goldens (tests/golden/packrgb_goldens.json), which reproduce from the committed crop."""
import json
from functools import lru_cache

import numpy as np

import fixtures as fx

U32 = np.uint32


def pack(r: np.ndarray, g: np.ndarray, b: np.ndarray, bits: int) -> np.ndarray:
    """bits 8: b | g << 8 | r << 16 | 255 << 24 (in memory B, G, R, 0xFF); bits 10: b | g << 10 | r << 20 | 3 << 30 in uint32 arithmetic: nothing is
    masked, a sample above 1023 runs into the next field and what is shifted beyond bit 31 is lost"""
    want, sh, top = {8: (np.uint8, 8, U32(255) << U32(24)), 10: (np.uint16, 10, U32(3) << U32(30))}[bits]
    assert r.dtype == g.dtype == b.dtype == want, (r.dtype, bits)
    return (b.astype(U32) | (g.astype(U32) << U32(sh)) | (r.astype(U32) << U32(2 * sh)) | top).astype(U32)


def rgb30(rgb24: np.ndarray) -> np.ndarray:
    """zimg's full-range 8 -> 10 bit conversion (what the reference's make_clip does for RGB30)"""
    return np.floor(rgb24.astype(np.float64) * 1023.0 / 255.0 + 0.5).astype(np.uint16)


def geometry(a: np.ndarray, name: str) -> np.ndarray:
    """the reference's clip geometries (tests/conftest.py) on planes stacked in axis 0"""
    if name == "full":
        return a
    if name == "odd":
        return np.ascontiguousarray(a[:, :-1, :-1])
    if name == "tiny":
        return np.ascontiguousarray(a[:, 100:107, 200:213])
    raise ValueError(name)


def golden_inputs(fmt: str, geom: str):
    """-> (r, g, b planes, bits) of the golden key `fmt|geom|default`"""
    rgb = fx.crop_rgb24()
    a, bits = (rgb, 8) if fmt == "RGB24" else (rgb30(rgb), 10)
    r, g, b = geometry(a, geom)
    return np.ascontiguousarray(r), np.ascontiguousarray(g), np.ascontiguousarray(b), bits


def stats(packed: np.ndarray) -> dict:
    """the reference's statistic: std.PlaneStats over the packed plane seen as a four times wider plane of bytes"""
    return fx.plane_stats(np.ascontiguousarray(packed).view(np.uint8))


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "packrgb_goldens.json").read_text())


def gpu_plane(seed: int, w: int, h: int, dtype) -> np.ndarray:
    """even seeds: natural content (the crop tiled), odd seeds: noise over the sample type's whole range"""
    if seed % 2 == 0:
        return fx.tiled_natural((h, w), dtype, (seed // 2) % 3)
    return fx.splitmix64_plane(seed, (h, w), dtype)


def gpu_frame(seed: int, w: int, h: int, bits: int):
    """r, g, b of one frame. bits 10: natural content is on the 10-bit scale; noise covers all 16 bits, so samples above 1023 are in"""
    dt = np.uint8 if bits == 8 else np.uint16
    planes = [gpu_plane(seed + 2 * k if seed % 2 == 0 else seed + 2 * k + 100, w, h, dt) for k in range(3)]
    if bits == 10 and seed % 2 == 0:
        planes = [(p >> 6).astype(np.uint16) for p in planes]
    return [np.ascontiguousarray(p) for p in planes]
