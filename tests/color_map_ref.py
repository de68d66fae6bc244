"""vszip.ColorMap in numpy: the table build with the reference's roundings (src/vapoursynth/color_map.zig:92-103) and the per-sample
lookup, the spec the library's vszip_color_map_lut and the device are compared with; the four palettes that are public formulas; and
the inputs of the five reference goldens that need nothing else (tests/golden/colormap_goldens.json)."""
import json
from functools import lru_cache

import numpy as np

import fixtures as fx

F32 = np.float32

# length of the reference's tables, plus the edges
LENGTHS = [1, 2, 9, 11, 64, 256, 257, 510]
# name -> (the reference's `color` index, points)
ANALYTIC = {"autumn": (0, 64), "winter": (3, 11), "spring": (7, 64), "cool": (8, 64)}


def lut(r, g, b, contracted: bool = False) -> np.ndarray:
    """(3, 256) uint8. Every operation is rounded to f32 on its own, except the final multiply-add, which is one fused operation (emulated in
    f64, where v * 255 + 0.5 is exact). contracted = True: the interpolation as a compiler that fuses d * frac + lo would compute it (what the
    library must NOT do). Raises ValueError where the reference's @trunc to u8 is undefined."""
    pal = np.stack([np.asarray(c, F32).reshape(-1) for c in (r, g, b)])
    n = pal.shape[1]
    if n < 1:
        raise ValueError("len = 0")
    i = np.arange(256, dtype=F32)
    p = (i * F32(n - 1)) / F32(255.0)
    lo = np.floor(p).astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    frac = (p - lo.astype(F32)).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (pal[:, hi] - pal[:, lo]).astype(F32)
        if contracted:
            v = (d.astype(np.float64) * frac.astype(np.float64) + pal[:, lo].astype(np.float64)).astype(F32)
        else:
            v = (pal[:, lo] + (d * frac).astype(F32)).astype(F32)
        t = (v.astype(np.float64) * 255.0 + 0.5).astype(F32)
    bad = ~((t > F32(-1.0)) & (t < F32(256.0)))
    if bad.any():
        c, k = np.argwhere(bad)[0]
        raise ValueError(f"{'rgb'[c]}: table entry {k}")
    return np.trunc(t).astype(np.uint8)


def apply(src: np.ndarray, table: np.ndarray):
    """-> r, g, b"""
    assert src.dtype == np.uint8 and table.shape == (3, 256) and table.dtype == np.uint8
    return table[0][src], table[1][src], table[2][src]


def analytic_palette(name: str):
    """r, g, b of the maps whose points are a formula of t = k / (points - 1), as f32 ramps: autumn (1, t, 0), winter (0, t, 1 - t / 2),
    spring (1, t, 1 - t), cool (t, 1 - t, 1)"""
    n = ANALYTIC[name][1]
    t = (np.arange(n, dtype=np.float64) / (n - 1)).astype(F32)
    one, zero = np.ones(n, F32), np.zeros(n, F32)
    return {"autumn": (one, t, zero), "winter": (zero, t, (1.0 - t.astype(np.float64) / 2.0).astype(F32)), "spring": (one, t, (F32(1.0) - t).astype(F32)),
            "cool": (t, (F32(1.0) - t).astype(F32), one)}[name]


def palette_of_color(color: int):
    return analytic_palette({v[0]: k for k, v in ANALYTIC.items()}[color])


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "colormap_goldens.json").read_text())


def golden_input(key: str):
    """-> (the Gray8 plane, the `color` index) of a key `GRAY8|geometry|color=N`"""
    fmt, geom, arg = key.split("|")
    assert fmt == "GRAY8" and arg.startswith("color=")
    y = fx.crop_gray8()
    y = {"full": y, "odd": y[:-1, :-1], "tiny": y[100:107, 200:213]}[geom]
    return np.ascontiguousarray(y), int(arg[6:])


def gpu_plane(seed: int, w: int, h: int) -> np.ndarray:
    """seed % 3 == 0: natural content, 1: noise, 2: every value 0..255 in turn (the rows start at different values)"""
    if seed % 3 == 0:
        return np.ascontiguousarray(fx.tiled_natural((h, w), np.uint8, (seed // 3) % 3))
    if seed % 3 == 1:
        return np.ascontiguousarray(fx.splitmix64_plane(seed, (h, w), np.uint8))
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + 37 * yy + seed) & 255).astype(np.uint8)


def permutation_lut(seed: int = 0) -> np.ndarray:
    """three distinct random permutations of 0..255: a swapped channel or an index off by one cannot pass"""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8)
    assert not any(np.array_equal(t[a], t[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    return np.ascontiguousarray(t)
