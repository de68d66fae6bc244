"""The numpy spec of vszip_depth_fmt (tests/depth_fmt_ref.py) against what pins it (no GPU): oracle/vs_host.py int_to_float / float_to_int, the
zimg steps the reference's goldens pass through, bit for bit over every bits in {8, 9, 10, 12, 16} x {limited, full} x {luma, chroma} (every code
value for 8 and 10 bits, seeded noise plus the extremes beyond); tests/depth_ref.py for integer -> integer; and the properties the GPU tests lean
on: the content holds ties, clamped runs, Inf, signed zeros and half subnormals."""
import numpy as np
import pytest

import depth_fmt_ref as df
import depth_ref as dr
import fixtures as fx
from oracle import vs_host as vh

BITS = (8, 9, 10, 12, 16)
CASES = [(full, chroma) for full in (False, True) for chroma in (False, True)]


def codes(bits):
    if bits <= 10:
        a = np.arange(1 << bits)
    else:
        a = np.concatenate([fx.splitmix64_plane(bits, (64, 64), np.uint16).reshape(-1) >> np.uint16(16 - bits), [0, 1, (1 << bits) - 2, (1 << bits) - 1, 1 << (bits - 1), 16 << (bits - 8)]])
    return a.astype(dr.dtype_of(bits)).reshape(1, -1)


def floats(bits, full, chroma):
    """every code value's float (and the points a quarter and a half step around it) for 8 and 10 bits, noise beyond; the range overshot at both ends"""
    off, rng = df.range_of(bits, full, chroma)
    if bits <= 10:
        q = np.arange(-8, (1 << bits) + 8, 0.25)
    else:
        q = np.concatenate([fx.splitmix64_plane(bits + 1, (64, 64), np.uint16).reshape(-1).astype(np.float64) / 65535.0 * ((1 << bits) + 16) - 8,
                            np.arange(-2, 3, 0.5), (1 << bits) - 1 + np.arange(-2, 3, 0.5)])
    return ((q - off) / rng).astype(np.float32).reshape(1, -1)


@pytest.mark.parametrize("full,chroma", CASES)
@pytest.mark.parametrize("bits", BITS)
def test_int_to_float_is_vs_hosts(bits, full, chroma):
    v = codes(bits)
    got, want = df.int_to_float(v, bits, full, chroma), vh.int_to_float(v, bits, not full, chroma)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    out = df.convert(v, df.dtype_for_bits(bits), bits, df.F32, 32, df.NONE, full, chroma)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    half = df.convert(v, df.dtype_for_bits(bits), bits, df.F16, 16, df.NONE, full, chroma)
    assert half.dtype == np.float16 and np.array_equal(half.view(np.uint16), want.astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("full,chroma", CASES)
@pytest.mark.parametrize("bits", BITS)
def test_float_to_int_is_vs_hosts(bits, full, chroma):
    x = floats(bits, full, chroma)
    got, want = df.float_to_int(x, bits, full, chroma), vh.float_to_int(x, bits, not full, chroma)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert got.min() == 0 and got.max() == (1 << bits) - 1  # both clamps are reached
    assert np.array_equal(df.convert(x, df.F32, 32, df.dtype_for_bits(bits), bits, df.NONE, full, chroma), want)
    inf = np.array([[np.inf, -np.inf]], np.float32)
    assert df.float_to_int(inf, bits, full, chroma).tolist() == [[(1 << bits) - 1, 0]]


@pytest.mark.parametrize("full,chroma", CASES)
@pytest.mark.parametrize("bits", (8, 10, 16))
def test_round_trip_returns_every_code_value(bits, full, chroma):
    v = codes(bits)
    assert np.array_equal(df.float_to_int(df.int_to_float(v, bits, full, chroma), bits, full, chroma), v)


@pytest.mark.parametrize("bits_in,bits_out,dither,full", [(16, 8, 1, False), (16, 10, 1, True), (10, 8, 1, False), (8, 16, 0, False), (8, 16, 0, True), (16, 8, 0, False), (12, 12, 0, True)])
def test_integer_to_integer_is_depth_ref(bits_in, bits_out, dither, full):
    a = dr.content(5, 37, 53, bits_in)
    got = df.convert(a, df.dtype_for_bits(bits_in), bits_in, df.dtype_for_bits(bits_out), bits_out, dither, full)
    want = dr.convert(a, bits_in, bits_out, dither, full)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    with pytest.raises(dr.DepthError, match="Depth: plane 0: full-range chroma is not built") as e:
        df.convert(a, df.dtype_for_bits(bits_in), bits_in, df.dtype_for_bits(bits_out), bits_out, dither, True, True)
    assert e.value.code == df.ERR_UNSUPPORTED


def test_float_diffusion_is_the_serial_recurrence():
    """the fast builder on float samples against depth_ref's serial one, with scale = rng; the clamp holds and feeds the error"""
    for bits, half in ((8, False), (10, False), (16, False), (8, True)):
        a = df.content(3, 23, 41, bits, True, False, half)
        got = df.convert(a, df.F16 if half else df.F32, 16 if half else 32, df.dtype_for_bits(bits), bits, df.ERROR_DIFFUSION, True)
        with np.errstate(invalid="ignore"):
            want = dr._diffuse_serial(a.astype(np.float32), np.float32((1 << bits) - 1), np.float32((1 << bits) - 1)).astype(got.dtype)
        assert np.array_equal(got, want), bits
        assert got.min() == 0 and got.max() == (1 << bits) - 1
        assert not np.array_equal(got, df.convert(a, df.F16 if half else df.F32, 16 if half else 32, df.dtype_for_bits(bits), bits, df.NONE, True))


@pytest.mark.parametrize("full,chroma", CASES)
@pytest.mark.parametrize("bits", (8, 10, 16))
def test_the_content_holds_what_the_gpu_tests_need(bits, full, chroma):
    a = df.content(1, 40, 60, bits, full, chroma)
    assert a.dtype == np.float32 and not np.isnan(a).any()
    off, rng = df.range_of(bits, full, chroma)
    y = vh.fma32(np.where(np.isfinite(a), a, 0), np.float32(rng), np.float32(off)).astype(np.float64)
    ties = (y - np.floor(y) == 0.5) & (y > 0) & (y < (1 << bits) - 1)
    assert ties.sum() >= 20, ties.sum()  # exact ties: half to even decides them
    assert (y < 0).sum() >= 20 and (y > (1 << bits) - 1).sum() >= 20
    assert np.isposinf(a).any() and np.isneginf(a).any() and (np.signbit(a) & (a == 0)).any()
    h = df.content(1, 40, 60, bits, full, chroma, half=True)
    assert h.dtype == np.float16 and ((h != 0) & (np.abs(h.astype(np.float32)) < 2.0**-14)).any()  # half subnormals survive


def test_half_rounding_is_nearest_even_with_subnormals():
    x = np.array([[1.0 + 2.0**-11, 1.0 + 3 * 2.0**-11, 2.0**-24 * 1.5, 2.0**-25, 65520.0, -65520.0, 65519.0, 2.0**-14 * (1 - 2.0**-11)]], np.float32)
    want = np.array([[1.0, 1.0 + 2.0**-9, 2.0**-23, 0.0, np.inf, -np.inf, 65504.0, 2.0**-14]], np.float16)
    assert np.array_equal(df.convert(x, df.F32, 32, df.F16, 16).view(np.uint16), want.view(np.uint16))
    # the code value one above black of a 16-bit limited plane is a half subnormal
    v = np.array([[4097]], np.uint16)
    h = df.convert(v, df.U16, 16, df.F16, 16)
    assert 0 < float(h[0, 0]) < 2.0**-14


def test_check_args_texts():
    pl = [(True, True, 8, 8, 8, 8, False)]
    for args, code, msg in [((4, 8, df.F32, 32, 0, 0, pl), -1, "DepthFmt: dtype_in 4 is none of VSZIP_U8, VSZIP_U16, VSZIP_F16, VSZIP_F32"),
                            ((df.U8, 8, -1, 32, 0, 0, pl), -1, "DepthFmt: dtype_out -1 is none of VSZIP_U8, VSZIP_U16, VSZIP_F16, VSZIP_F32"),
                            ((df.U16, 8, df.F32, 32, 0, 0, pl), -1, "DepthFmt: bits_in 8 does not fit VSZIP_U16 (9..16)"),
                            ((df.U8, 8, df.F32, 16, 0, 0, pl), -1, "DepthFmt: bits_out 16 does not fit VSZIP_F32 (32)"),
                            ((df.F32, 32, df.U8, 8, 2, 0, pl), -1, "DepthFmt: dither 2 is neither 0 (none) nor 1 (error diffusion)"),
                            ((df.U8, 8, df.F16, 16, 1, 0, pl), -1, "DepthFmt: error diffusion needs an integer destination, dtype_out is VSZIP_F16"),
                            ((df.F32, 32, df.U8, 8, 0, 0, []), -1, "DepthFmt: no planes"),
                            ((df.F32, 32, df.U8, 8, 0, 0, [(True, False, 8, 8, 8, 8, False)]), -1, "DepthFmt: plane 0: src and dst must not be NULL"),
                            ((df.F32, 32, df.U8, 8, 0, 0, pl + [(True, True, 8, 8, 8, 4, False)]), -1, "DepthFmt: plane 1: bad geometry 8x8, pitches 8 -> 4"),
                            ((df.F32, 32, df.U8, 8, 1, 0, pl), -3, "DepthFmt: plane 0: error diffusion from float with an offset (limited range) is not built (DESIGN.md section 1)"),
                            ((df.F32, 32, df.U8, 8, 1, 1, pl + [(True, True, 8, 8, 8, 8, True)]), -3,
                             "DepthFmt: plane 1: error diffusion from float with an offset (chroma) is not built (DESIGN.md section 1)"),
                            ((df.U16, 16, df.U8, 8, 1, 1, [(True, True, 8, 8, 8, 8, True)]), -3, "Depth: plane 0: full-range chroma is not built (DESIGN.md section 1)")]:
        with pytest.raises(dr.DepthError) as e:
            df.check_args(*args)
        assert (e.value.code, str(e.value)) == (code, msg)
    df.check_args(df.F32, 32, df.U8, 8, 1, 1, pl)
    df.check_args(df.F32, 32, df.U8, 8, 0, 0, [(True, True, 8, 8, 8, 8, True)])
