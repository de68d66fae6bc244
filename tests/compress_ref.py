"""Parity spec of vszip.Compress in numpy: the MPEG-2 / JPEG intra round trip of every 8 x 8 block of an 8-bit plane. What the
create function of src/vapoursynth/compress.zig checks and QuantTables.buildMpeg2 / buildJpeg derive (tables()), and what
processPlane of src/filters/compress.zig computes per block (plane()): level shift, the "islow" forward DCT in two passes,
quantise, dequantise, the "simple" inverse DCT in two passes, clamp.

Formulation. All blocks of a plane go through each stage together as an (N, 8, 8) int32 array. int32 array arithmetic in numpy
wraps, as the reference's +% -% *% do; `trunc16` is the truncation to i16 that every pass applies when it stores its block. The
quantiser's products are made in int64 (a coefficient reaches 2^14, a multiplier 2^18), the deadzone compare in uint64. A partial
block at the right or bottom edge replicates the last column / row of the plane and stores only what lies inside it.

Two conditionals of the reference only skip adding zeros (m4|m5|m6|m7 in the row pass, c4..c7 != 0 in the column pass) and are not
restated. The third is kept, because it changes bits: a row whose columns 1..7 are all zero becomes trunc16(8 c0) eight times.
"""
from __future__ import annotations

import json
from functools import lru_cache

import numpy as np

import fixtures as fx

I32, I64 = np.int32, np.int64
DEFAULTS = dict(codec=0, qscale=8, dc_prec=0, quality=50)

# quantisation matrices in natural raster order: MPEG-1/2 default intra (luma and chroma), JPEG Annex K luminance, chrominance
MPEG_INTRA = np.array([
    8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
    22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83], I64)
JPEG_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], I64)
JPEG_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, I64)

QMAT_SHIFT = 21
MPEG_BIAS = 96 << 13                           # the intra bias 3/8, in units of 2^-21
MPEG_T1 = (1 << QMAT_SHIFT) - MPEG_BIAS - 1     # deadzone: |coef qmul| <= T1 quantises to zero
JPEG_BIAS = 1 << (QMAT_SHIFT - 1)               # round to nearest, symmetric

FIX = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
           f2_053=16819, f2_562=20995, f3_072=25172)
W1, W2, W3, W4, W5, W6, W7 = 22725, 21407, 19266, 16383, 12873, 8867, 4520
ROW_SHIFT, COL_SHIFT = 11, 20
COL_DC_BIAS = (1 << (COL_SHIFT - 1)) // W4  # 32


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def tables(codec=0, qscale=8, dc_prec=0, quality=50) -> dict:
    """compressCreate's checks in its order (only the chosen codec's parameters), then buildMpeg2 | buildJpeg.
    -> codec, qmul[2][64], deq[2][64] (int32; [0] luma, [1] chroma), dc_q, dc_scale"""
    if codec < 0 or codec > 1:
        raise ValueError("Compress: codec must be 0 (mpeg2) or 1 (jpeg).")
    qmul, deq = np.zeros((2, 64), I32), np.zeros((2, 64), I32)
    dc_q, dc_scale = 64, 8
    if codec == 0:
        if qscale < 1 or qscale > 31:
            raise ValueError("Compress: qscale must be between 1 and 31.")
        if dc_prec < 0 or dc_prec > 3:
            raise ValueError("Compress: dc_prec must be between 0 and 3.")
        den = (int(qscale) << 1) * MPEG_INTRA
        qmul[:] = ((2 << QMAT_SHIFT) // den).astype(I32)
        deq[:] = den.astype(I32)
        dc_scale = 8 >> int(dc_prec)
        dc_q = dc_scale << 3
    else:
        if quality < 1 or quality > 100:
            raise ValueError("Compress: quality must be between 1 and 100.")
        scale = 5000 // int(quality) if quality < 50 else 200 - int(quality) * 2
        for p, base in enumerate((JPEG_LUMA, JPEG_CHROMA)):
            q = np.clip((base * scale + 50) // 100, 1, 255)
            deq[p] = q.astype(I32)
            qmul[p] = ((1 << QMAT_SHIFT) // (8 * q)).astype(I32)
    return dict(codec=int(codec), qmul=qmul, deq=deq, dc_q=int(dc_q), dc_scale=int(dc_scale))


# ---- the block pipeline -----------------------------------------------------------------------------------------------------------
def trunc16(a: np.ndarray) -> np.ndarray:
    return a.astype(np.int16).astype(I32)


def _descale(x, n):
    return (x + I32(1 << (n - 1))) >> n


def _fdct1d(t, out_round, even_shift):
    """t: eight int32 arrays; even_shift < 0: the first pass (even outputs scaled by 2^4)"""
    c = {k: I32(v) for k, v in FIX.items()}
    tmp0, tmp7, tmp1, tmp6 = t[0] + t[7], t[0] - t[7], t[1] + t[6], t[1] - t[6]
    tmp2, tmp5, tmp3, tmp4 = t[2] + t[5], t[2] - t[5], t[3] + t[4], t[3] - t[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    o = [None] * 8
    if even_shift < 0:
        o[0], o[4] = (tmp10 + tmp11) * I32(16), (tmp10 - tmp11) * I32(16)
    else:
        o[0], o[4] = _descale(tmp10 + tmp11, even_shift), _descale(tmp10 - tmp11, even_shift)
    z1 = (tmp12 + tmp13) * c["f0_541"]
    o[2] = _descale(z1 + tmp13 * c["f0_765"], out_round)
    o[6] = _descale(z1 + tmp12 * -c["f1_847"], out_round)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * c["f1_175"]
    o4, o5, o6, o7 = tmp4 * c["f0_298"], tmp5 * c["f2_053"], tmp6 * c["f3_072"], tmp7 * c["f1_501"]
    z1, z2 = z1 * -c["f0_899"], z2 * -c["f2_562"]
    z3, z4 = z3 * -c["f1_961"] + z5, z4 * -c["f0_390"] + z5
    o[7], o[5], o[3], o[1] = (_descale(o4 + (z1 + z3), out_round), _descale(o5 + (z2 + z4), out_round), _descale(o6 + (z2 + z3), out_round),
                              _descale(o7 + (z1 + z4), out_round))
    return o


def fdct(b: np.ndarray) -> np.ndarray:
    """(N, 8, 8) int32 samples -> coefficients with the overall factor 8, truncated to i16 after each pass"""
    b = trunc16(np.stack(_fdct1d([b[:, :, k] for k in range(8)], 13 - 4, -1), axis=2))
    return trunc16(np.stack(_fdct1d([b[:, k, :] for k in range(8)], 13 + 4, 4), axis=1))


def _tdiv(a, b):
    """division truncated toward zero"""
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def quant_dequant(b: np.ndarray, tb: dict, idx: int, counts: dict | None = None) -> np.ndarray:
    n = b.shape[0]
    c = b.reshape(n, 64)
    prod = c.astype(I64) * tb["qmul"][idx].astype(I64)
    d = tb["deq"][idx].astype(I32)
    if tb["codec"] == 0:
        kept = (prod + I64(MPEG_T1)).view(np.uint64) > np.uint64(2 * MPEG_T1)
        lvl = np.where(prod > 0, (I64(MPEG_BIAS) + prod) >> QMAT_SHIFT, -((I64(MPEG_BIAS) - prod) >> QMAT_SHIFT))
        lvl = np.where(kept, lvl, 0).astype(I32)
        lvl[:, 0] = _tdiv(c[:, 0] + I32(tb["dc_q"] >> 1), I32(tb["dc_q"]))
        mag = (np.abs(lvl) * d) >> 4  # the magnitude is dequantised, then the sign restored
        out = trunc16(np.where(lvl < 0, -mag, mag))
        out[:, 0] = trunc16(lvl[:, 0] * I32(tb["dc_scale"]))
        ac = slice(1, 64)
    else:
        lvl = np.where(prod > 0, (I64(JPEG_BIAS) + prod) >> QMAT_SHIFT, np.where(prod < 0, -((I64(JPEG_BIAS) - prod) >> QMAT_SHIFT), 0)).astype(I32)
        out = trunc16(lvl * d)
        ac = slice(0, 64)
    if counts is not None:
        _add(counts, "killed", ((c[:, ac] != 0) & (lvl[:, ac] == 0)).sum())
        _add(counts, "kept", (lvl[:, ac] != 0).sum())
        _add(counts, "positive", (lvl[:, ac] > 0).sum())
        _add(counts, "negative", (lvl[:, ac] < 0).sum())
    return out.reshape(n, 8, 8)


def idct(b: np.ndarray, offset: int, counts: dict | None = None) -> np.ndarray:
    """(N, 8, 8) coefficients -> (N, 8, 8) uint8"""
    c = [b[:, :, k] for k in range(8)]
    dc_only = (c[1] | c[2] | c[3] | c[4] | c[5] | c[6] | c[7]) == 0
    a0 = I32(W4) * c[0] + I32(1 << (ROW_SHIFT - 1))
    a = [a0 + I32(W2) * c[2], a0 + I32(W6) * c[2], a0 - I32(W6) * c[2], a0 - I32(W2) * c[2]]
    e = [I32(W1) * c[1] + I32(W3) * c[3], I32(W3) * c[1] - I32(W7) * c[3], I32(W5) * c[1] - I32(W1) * c[3], I32(W7) * c[1] - I32(W5) * c[3]]
    a[0] = a[0] + (I32(W4) * c[4] + I32(W6) * c[6])
    a[1] = a[1] + (I32(-W4) * c[4] - I32(W2) * c[6])
    a[2] = a[2] + (I32(-W4) * c[4] + I32(W2) * c[6])
    a[3] = a[3] + (I32(W4) * c[4] - I32(W6) * c[6])
    e[0] = e[0] + (I32(W5) * c[5] + I32(W7) * c[7])
    e[1] = e[1] + (I32(-W1) * c[5] - I32(W5) * c[7])
    e[2] = e[2] + (I32(W7) * c[5] + I32(W3) * c[7])
    e[3] = e[3] + (I32(W3) * c[5] - I32(W1) * c[7])
    row = [None] * 8
    for k in range(4):
        row[k], row[7 - k] = trunc16((a[k] + e[k]) >> ROW_SHIFT), trunc16((a[k] - e[k]) >> ROW_SHIFT)
    dc = trunc16(c[0] * I32(8))
    r = np.stack([np.where(dc_only, dc, v) for v in row], axis=2)
    if counts is not None:
        _add(counts, "dc_only_row", dc_only.sum())
        _add(counts, "general_row", (~dc_only).sum())
    c = [r[:, k, :] for k in range(8)]
    a0 = I32(W4) * (c[0] + I32(COL_DC_BIAS))
    a = [a0 + I32(W2) * c[2], a0 + I32(W6) * c[2], a0 - I32(W6) * c[2], a0 - I32(W2) * c[2]]
    e = [I32(W1) * c[1] + I32(W3) * c[3], I32(W3) * c[1] - I32(W7) * c[3], I32(W5) * c[1] - I32(W1) * c[3], I32(W7) * c[1] - I32(W5) * c[3]]
    a[0] = a[0] + I32(W4) * c[4] + I32(W6) * c[6]
    a[1] = a[1] - I32(W4) * c[4] - I32(W2) * c[6]
    a[2] = a[2] - I32(W4) * c[4] + I32(W2) * c[6]
    a[3] = a[3] + I32(W4) * c[4] - I32(W6) * c[6]
    e[0] = e[0] + I32(W5) * c[5] + I32(W7) * c[7]
    e[1] = e[1] - I32(W1) * c[5] - I32(W5) * c[7]
    e[2] = e[2] + I32(W7) * c[5] + I32(W3) * c[7]
    e[3] = e[3] + I32(W3) * c[5] - I32(W1) * c[7]
    col = [None] * 8
    for k in range(4):
        col[k], col[7 - k] = ((a[k] + e[k]) >> COL_SHIFT) + I32(offset), ((a[k] - e[k]) >> COL_SHIFT) + I32(offset)
    v = np.stack(col, axis=1)
    if counts is not None:
        _add(counts, "clamped_0", (v < 0).sum())
        _add(counts, "clamped_255", (v > 255).sum())
    return np.clip(v, 0, 255).astype(np.uint8)


def _add(counts: dict, key: str, n) -> None:
    counts[key] = counts.get(key, 0) + int(n)


def plane(src: np.ndarray, tb: dict, chroma: bool = False, counts: dict | None = None) -> np.ndarray:
    """processPlane: src (h, w) uint8; counts: a dict that receives how often each branch was taken"""
    assert src.dtype == np.uint8 and src.ndim == 2
    h, w = src.shape
    by, bx = -(-h // 8), -(-w // 8)
    ys, xs = np.minimum(np.arange(by * 8), h - 1), np.minimum(np.arange(bx * 8), w - 1)
    level = 128 if tb["codec"] == 1 else 0
    b = (src[ys][:, xs].astype(I32) - I32(level)).reshape(by, 8, bx, 8).transpose(0, 2, 1, 3).reshape(by * bx, 8, 8)
    out = idct(quant_dequant(fdct(b), tb, 1 if chroma else 0, counts), level, counts)
    if counts is not None:
        _add(counts, "full_block", (h // 8) * (w // 8))
        _add(counts, "partial_x", by * (w % 8 != 0))
        _add(counts, "partial_y", bx * (h % 8 != 0))
    return np.ascontiguousarray(out.reshape(by, bx, 8, 8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)[:h, :w])


def frame(planes_in, chroma=True, **kw) -> list:
    """vszip.Compress on one frame: plane 0 with the luma tables, planes 1 and 2 with the chroma tables or, with chroma false, copied"""
    tb = tables(**dict(DEFAULTS, **kw))
    return [plane(p, tb, i != 0) if (i == 0 or chroma) else p.copy() for i, p in enumerate(planes_in)]


# ---- the reference's golden cases (tests/goldens/compress.json), rebuilt from tests/fixtures.py -----------------------------------
_FMT = {"GRAY8": None, "YUV420P8": (1, 1), "YUV422P8": (1, 0), "YUV444P8": (0, 0)}  # name -> (ssw, ssh)


@lru_cache(maxsize=None)
def goldens() -> dict:
    return json.loads((fx.GOLDEN_DIR / "compress_goldens.json").read_text())


def parse_key(key: str):
    """'YUV420P8|full|chroma=0,codec=0,qscale=20' -> (format, geometry, keyword arguments)"""
    fmt, geometry, args = key.split("|")
    kw = {k: int(v) for k, v in (it.split("=") for it in args.split(","))}
    if "chroma" in kw:
        kw["chroma"] = bool(kw["chroma"])
    return fmt, geometry, kw


@lru_cache(maxsize=None)
def _planes(fmt: str, geometry: str) -> tuple:
    ss = _FMT[fmt]
    if ss is None:
        g = fx.crop_gray8()
        p = [np.ascontiguousarray({"full": g, "odd": g[:-1, :-1], "tiny": g[100:107, 200:213]}[geometry])]
    else:
        p = fx.yuv_geometry(fx.crop_yuv(8, *ss), geometry, *ss)
    for x in p:
        x.setflags(write=False)
    return tuple(p)


def golden_inputs(fmt: str, geometry: str) -> list:
    return list(_planes(fmt, geometry))


def run_key(key: str) -> list:
    fmt, geometry, kw = parse_key(key)
    return frame(golden_inputs(fmt, geometry), **kw)


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (7, 13), (8, 8), (9, 9), (37, 83), (64, 72), (130, 67))  # (w, h)
MPEG2_PARAMS = tuple(dict(codec=0, qscale=q, dc_prec=d) for q in (1, 8, 31) for d in (0, 3))
JPEG_PARAMS = tuple(dict(codec=1, quality=q) for q in (1, 8, 50, 98, 100))


@lru_cache(maxsize=None)
def gpu_plane(seed: int, w: int, h: int) -> np.ndarray:
    """even seeds: full-range noise (every coefficient large, both clamps); odd seeds: natural content (smooth blocks: coefficients
    inside the deadzone, DC-only rows). tests/test_compress_ref.py counts the branches."""
    p = fx.splitmix64_plane(seed, (h, w), np.uint8) if seed % 2 == 0 else fx.tiled_natural((h, w), np.uint8, seed % 3)
    p = np.ascontiguousarray(p)
    p.setflags(write=False)
    return p


def gpu_planes(seed: int = 0) -> list:
    """one plane of every size in SIZES, noise and natural content alternating"""
    return [gpu_plane(seed + i, w, h) for i, (w, h) in enumerate(SIZES)]
