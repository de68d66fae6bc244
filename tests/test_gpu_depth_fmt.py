"""GPU: vszip_depth_fmt against the numpy spec (tests/depth_fmt_ref.py), bit for bit: integers as integers, floats by their uint32 / uint16
views; every operation is one correctly rounded IEEE operation on both sides, so there is no tolerance. `none` between integer (8, 10, 16 bits),
half and float planes for {limited, full} x {luma, chroma} on w in {1, 7, 15, 16, 17, 63, 64, 65, 130} x h in {1, 2, 5} (whole vectors, tails, single
columns); error diffusion from float and half to 8, 10 and 16 bits (full range, non-chroma) on w in {1, 2, 3, 63, 64, 65, 129} x h in {1, 2, 63, 64,
65, 129, 257}, both workgroup sizes each forced on the other's planes, 1030 x 40 (the carry row in LDS) and 260 x 4100 under the small workgroup
(the carry row in scratch). Content: noise beyond the range at both ends, clamped runs, exact ties, +-Inf, +-0, half subnormals, no NaN. Integer
-> integer equals vszip_depth byte for byte; bases and pitches off by one to three samples give the same bits; 200 planes in one call; the same
call twice; u8 -> f32 -> EEDI3 -> u8 on resident planes; every refusal with its code and text, dst untouched."""
from functools import lru_cache

import numpy as np
import pytest

import depth_fmt_ref as df
import depth_ref as dr
from test_gpu_depth import DIFFUSE, NONE
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu

U8, U16, F16, F32 = df.U8, df.U16, df.F16, df.F32
NONE_SIZES = [(h, w) for h in (1, 2, 5) for w in (1, 7, 15, 16, 17, 63, 64, 65, 130)]
DIFFUSE_SIZES = [(h, w) for h in (1, 2, 63, 64, 65, 129, 257) for w in (1, 2, 3, 63, 64, 65, 129)]
CASES = [(False, False), (False, True), (True, False), (True, True)]
CASE_IDS = ["limited-luma", "limited-chroma", "full-luma", "full-chroma"]
INT = {8: (U8, 8), 10: (U16, 10), 16: (U16, 16)}
FLT = {F16: (F16, 16), F32: (F32, 32)}


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def bits_of(a):
    return np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@lru_cache(maxsize=None)
def int_plane(seed, h, w, bits):
    a = dr.content(seed, h, w, bits)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def float_plane(seed, h, w, bits, full, chroma, half):
    a = df.content(seed, h, w, bits, full, chroma, half)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def want_from_float(seed, h, w, half, bits, dither, full, chroma):
    src = float_plane(seed, h, w, bits, full, chroma, half)
    a = df.convert(src, F16 if half else F32, 16 if half else 32, *INT[bits], dither, full, chroma)
    a.setflags(write=False)
    return a


def run(dev, srcs, tin, tout, dither=0, full=False, chroma=None, **opts):
    s = [dev.upload(a) for a in srcs]
    d = [dev.empty(a.shape[0], a.shape[1], df.NP[tout[0]]) for a in srcs]
    with dev.options(**opts):
        dev.depth_fmt(s, d, *tin, *tout, dither, full, chroma)
    return [dev.download(x) for x in d]


def same(got, want, *what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = bits_of(got) != bits_of(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def check_from_float(dev, sizes, fin, bits, dither, full=True, chroma=False, **opts):
    half = fin == F16
    outs = run(dev, [float_plane(i, h, w, bits, full, chroma, half) for i, (h, w) in enumerate(sizes)], FLT[fin], INT[bits], dither, full, chroma, **opts)
    for i, ((h, w), o) in enumerate(zip(sizes, outs)):
        same(o, want_from_float(i, h, w, half, bits, dither, full, chroma), h, w, fin, bits, dither, full, chroma, opts)


# ---- none -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full,chroma", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("fout", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("bits", [8, 10, 16])
def test_none_integer_to_float(dev, bits, fout, full, chroma):
    sizes = NONE_SIZES + [(3, 1000)]
    srcs = [int_plane(i, h, w, bits) for i, (h, w) in enumerate(sizes)]
    for a, o in zip(srcs, run(dev, srcs, INT[bits], FLT[fout], 0, full, chroma)):
        same(o, df.convert(a, *INT[bits], *FLT[fout], 0, full, chroma), a.shape, bits, fout, full, chroma)


@pytest.mark.parametrize("full,chroma", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("fin", [F32, F16], ids=["f32", "f16"])
def test_none_float_to_integer(dev, fin, bits, full, chroma):
    check_from_float(dev, NONE_SIZES + [(3, 1000)], fin, bits, df.NONE, full, chroma)


@pytest.mark.parametrize("fin,fout", [(F32, F16), (F16, F32), (F32, F32), (F16, F16)], ids=["f32-f16", "f16-f32", "f32-f32", "f16-f16"])
def test_none_float_to_float(dev, fin, fout):
    sizes = NONE_SIZES + [(3, 1000)]
    srcs = [float_plane(i, h, w, 16, False, False, fin == F16) for i, (h, w) in enumerate(sizes)]
    if fin == F32:  # the whole half range and beyond: overflow to Inf, the subnormals, the ties between neighbouring halves
        hb = np.arange(0, 0x7C00, 3, dtype=np.uint16)
        h, up = hb.view(np.float16).astype(np.float32), (hb + np.uint16(1)).view(np.float16).astype(np.float32)  # a half and the next one
        srcs.append(np.concatenate([h, -h, (h + up) / 2, np.float32([65519.9, 65520, 1e9, -1e9, 1e-9, -1e-9])]).astype(np.float32).reshape(3, -1))
    for a, o in zip(srcs, run(dev, srcs, FLT[fin], FLT[fout], 0, True)):  # full_range is ignored
        same(o, df.convert(a, *FLT[fin], *FLT[fout]), a.shape, fin, fout)


def test_luma_and_chroma_planes_in_one_call(dev):
    """the constants are each plane's own"""
    sizes = [(5, 130), (3, 65), (3, 65), (2, 17)]
    ch = [False, True, True, False]
    srcs = [int_plane(i, h, w, 8) for i, (h, w) in enumerate(sizes)]
    for a, c, o in zip(srcs, ch, run(dev, srcs, INT[8], FLT[F32], 0, False, ch)):
        same(o, df.convert(a, U8, 8, F32, 32, 0, False, c), a.shape, c)
    fl = [float_plane(i, h, w, 10, False, c, False) for i, ((h, w), c) in enumerate(zip(sizes, ch))]
    for a, c, o in zip(fl, ch, run(dev, fl, FLT[F32], INT[10], 0, False, ch)):
        same(o, df.convert(a, F32, 32, U16, 10, 0, False, c), a.shape, c)


# ---- error diffusion ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("fin", [F32, F16], ids=["f32", "f16"])
def test_error_diffusion(dev, fin, bits):
    check_from_float(dev, DIFFUSE_SIZES, fin, bits, df.ERROR_DIFFUSION)


@pytest.mark.parametrize("fin", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("waves", [4, 16])
def test_either_workgroup_on_every_size(dev, waves, fin):
    assert dev.get_option("VSZIP_DEPTH_WAVES") == 0
    check_from_float(dev, DIFFUSE_SIZES, fin, 8, df.ERROR_DIFFUSION, VSZIP_DEPTH_WAVES=waves)


@pytest.mark.parametrize("waves", [0, 4])
def test_more_rows_than_a_workgroup_holds(dev, waves):
    """1030 x 40: 17 bands on 16 waves, or on 4; the seam between the last wave and the first is the carry row in LDS"""
    check_from_float(dev, [(1030, 40)], F32, 8, df.ERROR_DIFFUSION, VSZIP_DEPTH_WAVES=waves)
    check_from_float(dev, [(1030, 40)], F16, 10, df.ERROR_DIFFUSION, VSZIP_DEPTH_WAVES=waves)


@pytest.mark.parametrize("fin,bits", [(F32, 8), (F16, 16)], ids=["f32-8", "f16-16"])
def test_the_carry_row_leaves_lds_for_scratch(dev, fin, bits):
    """260 x 4100 under the small workgroup: five bands on four waves, the fifth reads the carry row from the context's scratch"""
    check_from_float(dev, [(260, 4100)], fin, bits, df.ERROR_DIFFUSION, VSZIP_DEPTH_WAVES=4)


# ---- integer -> integer: vszip_depth itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("bits_in,bits_out,dither", [(a, b, 1) for a, b in DIFFUSE] + [(a, b, 0) for a, b in NONE])
def test_integer_to_integer_equals_vszip_depth(dev, bits_in, bits_out, dither, full):
    sizes = [(1, 1), (2, 17), (65, 129), (70, 203), (257, 33)]
    srcs = [dev.upload(int_plane(i, h, w, bits_in)) for i, (h, w) in enumerate(sizes)]
    a = [dev.empty(h, w, dr.dtype_of(bits_out)) for h, w in sizes]
    b = [dev.empty(h, w, dr.dtype_of(bits_out)) for h, w in sizes]
    dev.depth(srcs, a, bits_in, bits_out, dither, full)
    dev.depth_fmt(srcs, b, df.dtype_for_bits(bits_in), bits_in, df.dtype_for_bits(bits_out), bits_out, dither, full)
    for x, y, (h, w) in zip(a, b, sizes):
        assert np.array_equal(dev.download(x), dev.download(y)), (h, w)


# ---- alignment, batching, repeats ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tin,tout,dither", [((U8, 8), (F32, 32), 0), ((U16, 10), (F16, 16), 0), ((F32, 32), (U8, 8), 0), ((F16, 16), (U16, 16), 0), ((F32, 32), (F16, 16), 0),
                                             ((F16, 16), (F32, 32), 0), ((F32, 32), (U8, 8), 1), ((F16, 16), (U16, 10), 1)],
                         ids=["u8-f32", "u10-f16", "f32-u8", "f16-u16", "f32-f16", "f16-f32", "f32-u8-diffuse", "f16-u10-diffuse"])
def test_unaligned_bases_and_odd_pitches_give_the_same_bits(dev, tin, tout, dither):
    """every pointer one to three samples off a 16-byte boundary and every pitch odd, each in turn and both together"""
    h, w = 70, 203
    src = float_plane(3, h, w, tout[1] if tout[1] <= 16 else 8, True, False, tin[0] == F16) if df.is_float(tin[0]) else int_plane(3, h, w, tin[1])
    e = df.convert(src, *tin, *tout, dither, True)
    keep = []

    def shifted(a, shift, pitch):
        big = dev.empty(a.shape[0] + 1, pitch + 32, a.dtype)
        keep.append(big)
        v = dev.wrap(big.ptr + shift * a.itemsize, a.shape[0], a.shape[1], pitch, a.dtype)
        dev.copy_in(v, np.ascontiguousarray(a))
        dev.sync()
        return v
    for which in ("src", "dst", "all"):
        for shift in (1, 2, 3):
            on = lambda k: which in (k, "all")
            s = shifted(src, shift if on("src") else 0, 211 if on("src") else 224)
            d = shifted(np.zeros((h, w), df.NP[tout[0]]), shift if on("dst") else 0, 213 if on("dst") else 224)
            dev.depth_fmt([s], [d], *tin, *tout, dither, True)
            same(dev.download(d), e, which, shift)


def test_200_planes_of_mixed_sizes_in_one_call(dev):
    sizes = [(1 + (i * 7) % 71, 1 + (i * 13) % 97) for i in range(197)] + [(257, 33), (300, 5), (64, 300)]
    check_from_float(dev, sizes, F32, 8, df.ERROR_DIFFUSION)
    check_from_float(dev, sizes, F16, 10, df.NONE, False, True)
    srcs = [int_plane(i, h, w, 8) for i, (h, w) in enumerate(sizes)]
    for a, o in zip(srcs, run(dev, srcs, INT[8], FLT[F32], 0, False)):
        same(o, df.convert(a, U8, 8, F32, 32), a.shape)


def test_the_same_call_twice_gives_the_same_bytes(dev):
    sizes = [(129, 129), (1030, 40), (65, 300)]
    srcs = [dev.upload(float_plane(i, h, w, 8, True, False, False)) for i, (h, w) in enumerate(sizes)]
    dsts = [dev.empty(h, w, np.uint8) for h, w in sizes]
    call = dev.prepared_depth_fmt(srcs, dsts, F32, 32, U8, 8, df.ERROR_DIFFUSION, True)
    call()
    first = [dev.download(d) for d in dsts]
    call()
    for i, ((h, w), d, a) in enumerate(zip(sizes, dsts, first)):
        assert np.array_equal(dev.download(d), a), (h, w)
        same(a, want_from_float(i, h, w, False, 8, 1, True, False), h, w)


# ---- composition ------------------------------------------------------------------------------------------------------------------------------
def test_eedi3_on_an_8_bit_plane_without_a_host_step(dev):
    """u8 -> f32 (limited), vszip_eedi3 (field 1, dh), f32 -> u8 on resident planes equals the two conversions done in numpy around the same GPU
    EEDI3 call: the conversions are ordered on the stream with the filter between them"""
    import fixtures as fx
    from oracle import vs_host as vh

    src = fx.tiled_natural((32, 64), np.uint8)
    s8 = dev.upload(src)
    f = dev.empty(32, 64, np.float32)
    dev.depth_fmt([s8], [f], U8, 8, F32, 32)
    (mid,) = dev.eedi3([f], 1, dh=True)
    out = dev.empty(mid.h, mid.w, np.uint8)
    dev.depth_fmt([mid], [out], F32, 32, U8, 8)
    got = dev.download(out)
    (ref,) = dev.eedi3([dev.upload(vh.int_to_float(src, 8, True))], 1, dh=True)
    want = vh.float_to_int(dev.download(ref), 8, True)
    assert got.shape == (64, 64) and np.array_equal(got, want)
    assert len(np.unique(got)) > 16


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_dst_untouched(dev):
    f32 = dev.upload(float_plane(1, 8, 8, 8, True, False, False))
    u8, u16 = dev.upload(np.full((8, 8), 0xA5, np.uint8)), dev.upload(np.full((8, 8), 0xA5A5, np.uint16))
    o8, o16, of32 = dev.upload(np.full((8, 8), 0x5A, np.uint8)), dev.upload(np.full((8, 8), 0x5A5A, np.uint16)), dev.upload(np.full((8, 8), 7.0, np.float32))
    short = dev.wrap(o8.ptr, 8, 8, 4, np.uint8)
    for srcs, dsts, args, kw, code, msg in [
            ([f32], [o8], (4, 32, U8, 8), {}, -1, "DepthFmt: dtype_in 4 is none of VSZIP_U8, VSZIP_U16, VSZIP_F16, VSZIP_F32"),
            ([f32], [o8], (F32, 32, 7, 8), {}, -1, "DepthFmt: dtype_out 7 is none of VSZIP_U8, VSZIP_U16, VSZIP_F16, VSZIP_F32"),
            ([f32], [o8], (F32, 16, U8, 8), {}, -1, r"DepthFmt: bits_in 16 does not fit VSZIP_F32 \(32\)"),
            ([f32], [o16], (F32, 32, U16, 8), {}, -1, r"DepthFmt: bits_out 8 does not fit VSZIP_U16 \(9\.\.16\)"),
            ([f32], [o8], (F32, 32, U8, 8, 2), {}, -1, r"DepthFmt: dither 2 is neither 0 \(none\) nor 1 \(error diffusion\)"),
            ([u8], [of32], (U8, 8, F32, 32, 1), {}, -1, "DepthFmt: error diffusion needs an integer destination, dtype_out is VSZIP_F32"),
            ([], [], (F32, 32, U8, 8), {}, -1, "DepthFmt: no planes"),
            ([f32], [short], (F32, 32, U8, 8), {}, -1, "DepthFmt: plane 0: bad geometry 8x8, pitches 32 -> 4"),
            ([f32], [o8], (F32, 32, U8, 8, 1), {}, -3, r"DepthFmt: plane 0: error diffusion from float with an offset \(limited range\) is not built \(DESIGN.md section 1\)"),
            ([f32, f32], [o8, o8], (F32, 32, U8, 8, 1), dict(full_range=True, chroma=[False, True]), -3,
             r"DepthFmt: plane 1: error diffusion from float with an offset \(chroma\) is not built \(DESIGN.md section 1\)"),
            ([u16], [o8], (U16, 16, U8, 8, 1), dict(full_range=True, chroma=True), -3, r"Depth: plane 0: full-range chroma is not built \(DESIGN.md section 1\)"),
            ([u16], [o8], (U16, 16, U8, 8, 2), {}, -1, r"Depth: dither 2 is neither 0 \(none\) nor 1 \(error diffusion\)")]:
        with pytest.raises(VszipError, match=msg) as e:
            dev.depth_fmt(srcs, dsts, *args, **kw)
        assert e.value.code == code, msg
    with pytest.raises(ValueError, match="depth_fmt: destination planes are uint8"):
        dev.depth_fmt([f32], [o16], F32, 32, U8, 8)
    assert (dev.download(o8) == 0x5A).all() and (dev.download(o16) == 0x5A5A).all() and (dev.download(of32) == 7.0).all()
    dev.depth_fmt([f32], [o8], F32, 32, U8, 8, 1, full_range=True)  # served
    same(dev.download(o8), want_from_float(1, 8, 8, False, 8, 1, True, False))
