"""The pixel loop of vszip.ImageRead in numpy (copyPixels / copyPixelsIndexed of the reference's image_read.zig): the spec the device
(tests/test_gpu_image_unpack*.py) and the host build of the lane bodies (tests/test_image_unpack_body_host.py) are compared with, the
known answers of the reference's own tests (tests/golden/image_unpack_goldens.json), and the content generators of those tests."""
import json
from functools import lru_cache

import numpy as np

import fixtures as fx

GRAY, GRAY_ALPHA, RGB, RGBA, BGR, BGRA, INDEXED = range(7)
LAYOUT_NAMES = ["GRAY", "GRAY_ALPHA", "RGB", "RGBA", "BGR", "BGRA", "INDEXED"]
CHANNELS = {GRAY: 1, GRAY_ALPHA: 2, RGB: 3, RGBA: 4, BGR: 3, BGRA: 4, INDEXED: 1}  # samples a pixel in the packed source
HAS_ALPHA = {GRAY: False, GRAY_ALPHA: True, RGB: False, RGBA: True, BGR: False, BGRA: True, INDEXED: True}

# (layout, sample type, src_bits): the arms of the reference's switch, which the library must serve
COMBOS = ([(GRAY, np.uint8, b) for b in (1, 2, 4, 8)] + [(GRAY, np.uint16, 16), (GRAY_ALPHA, np.uint8, 8), (GRAY_ALPHA, np.uint16, 16), (RGB, np.uint8, 8), (BGR, np.uint8, 8),
          (RGBA, np.uint8, 8), (BGRA, np.uint8, 8), (RGB, np.uint16, 16), (RGBA, np.uint16, 16), (RGBA, np.float32, 32), (INDEXED, np.uint8, 8)])


def combo_id(combo) -> str:
    layout, dt, bits = combo
    return f"{LAYOUT_NAMES[layout]}-{np.dtype(dt).name}-{bits}"


def unpack(packed: np.ndarray, layout: int, src_bits: int = None, palette: np.ndarray = None, alpha: bool = True):
    """packed: (h, w, channels) samples in memory order ((h, w) is taken as one channel) -> ([p0] or [r, g, b], alpha plane or None).
    Samples pass as bits (floats included); grey below 8 bits: the low src_bits bits times 255 / (2^bits - 1); INDEXED: packed holds index
    bytes and palette is (256, 4) uint8 R, G, B, A. alpha=False drops the alpha plane."""
    a = packed[:, :, None] if packed.ndim == 2 else packed
    assert a.shape[2] == CHANNELS[layout], (a.shape, layout)
    bits = a.dtype.itemsize * 8 if src_bits is None else src_bits
    if layout == INDEXED:
        assert a.dtype == np.uint8 and bits == 8 and palette.shape == (256, 4) and palette.dtype == np.uint8
        ch = palette[a[:, :, 0]]  # (h, w, 4)
        return [np.ascontiguousarray(ch[:, :, c]) for c in range(3)], (np.ascontiguousarray(ch[:, :, 3]) if alpha else None)
    assert palette is None
    if bits < 8:
        assert layout == GRAY and a.dtype == np.uint8 and bits in (1, 2, 4)
        m = (1 << bits) - 1
        return [((a[:, :, 0] & np.uint8(m)).astype(np.uint32) * np.uint32(255 // m)).astype(np.uint8)], None
    assert bits == a.dtype.itemsize * 8
    ch = [np.ascontiguousarray(a[:, :, c]) for c in range(a.shape[2])]
    al = ch.pop() if HAS_ALPHA[layout] else None
    if layout in (BGR, BGRA):
        ch.reverse()  # planes are filled by name: R is the pixel's third sample
    return ch, (al if alpha else None)


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "image_unpack_goldens.json").read_text())


def golden_names() -> list:
    return sorted(k for k in goldens() if not k.startswith("_"))


def golden_case(name: str):
    """-> (packed array, layout, src_bits, palette or None, expected dict of p0 / p1 / p2 / a as arrays) of one golden entry"""
    g = goldens()[name]
    dt = np.dtype(g["dtype"])
    layout = LAYOUT_NAMES.index(g["layout"])
    packed = np.array(g["pixels"], dt)
    if packed.ndim == 2:
        packed = packed[:, :, None]
    pal = None
    if "palette" in g:
        pal = np.zeros((256, 4), np.uint8)
        pal[:, 3] = 255
        pal[:len(g["palette"]), :3] = np.array(g["palette"], np.uint8)
    want = {k: np.array(v, dt) for k, v in g["planes"].items()}
    return np.ascontiguousarray(packed), layout, g["src_bits"], pal, want


# ---- content of the GPU and host tests --------------------------------------------------------------------------------------------
def bits_of(a: np.ndarray) -> np.ndarray:
    """samples as unsigned integers of their width, for comparisons that see NaN payloads"""
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def content(seed: int, h: int, w: int, combo) -> np.ndarray:
    """(h, w, channels) noise over the sample type's whole range with 0 and the maximum put in where there is room; float: the bits of
    negative and positive values of every magnitude, with -Inf, +Inf, a quiet and a signalling NaN, -0.0 and a denormal put in; grey
    below 8 bits keeps its noise in the high bits, which the kernel has to ignore; INDEXED from 256 pixels on uses every index"""
    layout, dt, bits = combo
    c = CHANNELS[layout]
    dt = np.dtype(dt)
    if dt == np.float32:
        a = fx.splitmix64_plane(seed, (h, w * c * 2), np.uint16).astype(np.uint32)
        a = (a[:, 0::2] << np.uint32(16)) | a[:, 1::2]
        flat = a.reshape(-1)
        special = np.array([0xFF800000, 0x7F800000, 0x7FC00001, 0x7F800001, 0x80000000, 0x00000001, 0xFFFFFFFF, 0xBF800000], np.uint32)
        n = min(len(special), flat.size)
        flat[(np.arange(n) * 5) % flat.size] = special[:n]
        return a.reshape(h, w, c).view(np.float32)
    a = np.ascontiguousarray(fx.splitmix64_plane(seed, (h, w * c), dt)).reshape(-1)
    if a.size >= 2:
        a[(seed * 3) % a.size] = 0
        a[(seed * 3 + 1) % a.size] = np.iinfo(dt).max
    if layout == INDEXED and a.size >= 256:
        a[np.random.default_rng(seed).permutation(a.size)[:256]] = np.arange(256, dtype=np.uint8)
    return a.reshape(h, w, c)


def palette(seed: int = 0) -> np.ndarray:
    """(256, 4) uint8, every entry different from every other"""
    rng = np.random.default_rng(seed)
    v = rng.permutation(1 << 24)[:256].astype(np.uint32) | (rng.permutation(256).astype(np.uint32) << np.uint32(24))
    pal = np.stack([(v >> np.uint32(8 * k)) & np.uint32(255) for k in range(4)], axis=1).astype(np.uint8)
    assert len({tuple(e) for e in pal.tolist()}) == 256
    return np.ascontiguousarray(pal)


def row_bytes(packed: np.ndarray, pitch: int = None) -> np.ndarray:
    """the packed pixels as (h, pitch) bytes: dense, or with `pitch` bytes a row (padding 0xA5)"""
    h = packed.shape[0]
    dense = np.ascontiguousarray(packed).view(np.uint8).reshape(h, -1)
    if pitch is None or pitch == dense.shape[1]:
        return dense
    out = np.full((h, pitch), 0xA5, np.uint8)
    out[:, :dense.shape[1]] = dense
    return out
