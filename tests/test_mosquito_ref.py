"""CPU: the MosquitoNR parity spec (tests/mosquito_ref.py) reproduces every key of the reference's
tests/goldens/mosquito.json (tests/golden/mosquito_goldens.json) from tests/fixtures.py's inputs, restates the behavioural
tests of the reference's tests/test_mosquito.py, raises the wrapper's errors with its wording, shows that the inputs the
GPU suites reuse reach every direction class and both output clamps, and libvszip_hip.so exports the entry point.

The file holds 22 keys with 40 planes (13 one-plane keys, 9 three-plane keys)."""
import ctypes

import numpy as np
import pytest

import fixtures as fx
import mosquito_ref as mq

KEYS = sorted(mq.goldens())


def binary_noise(seed, shape, dtype, bits):
    """independent samples of 0 or the peak"""
    m = fx.splitmix64_plane(seed, shape, np.uint8) & 1
    return m.astype(np.float32) if np.dtype(dtype) == np.float32 else (m.astype(np.int64) * ((1 << bits) - 1)).astype(dtype)


def test_all_22_keys_are_committed():
    assert len(KEYS) == 22
    assert sum(len(v) for v in mq.goldens().values()) == 40
    assert {mq.parse_key(k)[0] for k in KEYS} == {"GRAY8", "GRAY10", "GRAY12", "GRAY14", "GRAY16", "GRAYS", "YUV420P8", "YUV420P16", "YUV444P16", "YUV444PS"}
    assert {mq.parse_key(k)[1] for k in KEYS} == {"full", "odd", "tiny"}


def test_parse_key():
    assert mq.parse_key("GRAY8|tiny|radius=2,restore=128,strength=16") == ("GRAY8", "tiny", dict(radius=2, restore=128, strength=16, which=(0,)))
    fmt, geo, kw = mq.parse_key("YUV444P16|full|planes=[0,1,2],radius=[2,1,2],restore=[128,64,96],strength=[16,8,24]")
    assert kw == dict(which=(0, 1, 2), radius=[2, 1, 2], restore=[128, 64, 96], strength=[16, 8, 24])
    assert mq.parse_key("YUV444P16|full|planes=[1,2],strength=16")[2] == dict(which=(1, 2), strength=16)


@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_golden(key):
    want = mq.goldens()[key]
    bits = mq.format_bits(mq.parse_key(key)[0])
    outs = mq.run_key(key)
    assert len(outs) == len(want)
    for i, o in enumerate(outs):
        st, g = mq.golden_stats(o, bits), want[f"p{i}"]
        if o.dtype.kind == "f":
            assert st["min"] == pytest.approx(g["min"], abs=1e-7, rel=0) and st["max"] == pytest.approx(g["max"], abs=1e-7, rel=0), (key, i, st, g)
        else:
            assert st["min"] == g["min"] and st["max"] == g["max"], (key, i, st, g)
        assert st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i, st, g)


# ---- the reference's behavioural tests ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yuv8():
    return mq.golden_inputs("YUV420P8", "full")


def test_strength0_is_exact_passthrough():
    for p in (fx.crop_gray8(), fx.crop_grays(), mq.golden_inputs("GRAY10", "full")[0]):
        assert np.array_equal(mq.mosquito_nr(p, 0, 128, 2, 10 if p.dtype == np.uint16 else None), p)


def test_default_planes_is_luma_only(yuv8):
    out = mq.mosquito_frame(yuv8, strength=16)
    assert not np.array_equal(out[0], yuv8[0]) and np.array_equal(out[1], yuv8[1]) and np.array_equal(out[2], yuv8[2])
    explicit = mq.mosquito_frame(yuv8, strength=16, which=(0,))
    assert all(np.array_equal(a, b) for a, b in zip(out, explicit))
    chroma = mq.mosquito_frame(yuv8, strength=16, which=(1, 2))
    assert np.array_equal(chroma[0], yuv8[0]) and not np.array_equal(chroma[1], yuv8[1]) and not np.array_equal(chroma[2], yuv8[2])


def test_scalar_equals_uniform_array_and_short_arrays_repeat_the_last(yuv8):
    all3 = dict(which=(0, 1, 2))
    a = mq.mosquito_frame(yuv8, 16, 64, 1, **all3)
    b = mq.mosquito_frame(yuv8, [16, 16, 16], [64, 64, 64], [1, 1, 1], **all3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    short = mq.mosquito_frame(yuv8, [16, 8], **all3)
    full = mq.mosquito_frame(yuv8, [16, 8, 8], **all3)
    assert all(np.array_equal(x, y) for x, y in zip(short, full))
    assert not np.array_equal(short[1], a[1])
    zero = mq.mosquito_frame(yuv8, [16, 0, 0], **all3)  # per-plane strength: 0 is a passthrough
    assert np.array_equal(zero[1], yuv8[1]) and np.array_equal(zero[2], yuv8[2]) and not np.array_equal(zero[0], yuv8[0])


def test_radius_and_restore_change_the_output():
    g = fx.crop_gray8()
    assert not np.array_equal(mq.mosquito_nr(g, 16, 128, 1), mq.mosquito_nr(g, 16, 128, 2))
    assert not np.array_equal(mq.mosquito_nr(g, 16, 0, 2), mq.mosquito_nr(g, 16, 128, 2))


def test_float_chroma_stays_in_its_range():
    out = mq.mosquito_frame(mq.golden_inputs("YUV444PS", "full"), strength=32, which=(0, 1, 2))
    for p in out[1:]:
        assert p.min() >= -0.5 and p.max() <= 0.5 and p.min() < 0
    assert out[0].min() >= 0.0 and out[0].max() <= 1.0


# ---- the create-time checks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,shape,msg", [
    (dict(strength=-1), (8, 8), r"MosquitoNR: strength value -1 is below minimum 0\."),
    (dict(strength=33), (8, 8), r"MosquitoNR: strength value 33 is above maximum 32\."),
    (dict(restore=-1), (8, 8), r"MosquitoNR: restore value -1 is below minimum 0\."),
    (dict(restore=129), (8, 8), r"MosquitoNR: restore value 129 is above maximum 128\."),
    (dict(radius=0), (8, 8), r"MosquitoNR: radius value 0 is below minimum 1\."),
    (dict(radius=3), (8, 8), r"MosquitoNR: radius value 3 is above maximum 2\."),
    (dict(strength=[16, 33, 16]), (8, 8), r"MosquitoNR: strength value 33 is above maximum 32\."),
    (dict(radius=[2, 2, 0]), (8, 8), r"MosquitoNR: radius value 0 is below minimum 1\."),
    (dict(strength=[16, 16, 16, 99]), (8, 8), r"MosquitoNR: strength has too many elements \(got 4, max 3\)\."),
    (dict(restore=[0, 0, 0, 0]), (8, 8), r"MosquitoNR: restore has too many elements \(got 4, max 3\)\."),
    (dict(), (3, 8), r"MosquitoNR: input is too small \(need at least 4x4 per processed plane\)\."),
    (dict(), (8, 3), r"MosquitoNR: input is too small \(need at least 4x4 per processed plane\)\."),
    # the order of the checks: size, strength, restore, radius
    (dict(strength=99, restore=-1, radius=0), (3, 3), "too small"),
    (dict(strength=99, restore=-1, radius=0), (8, 8), "strength value 99"),
    (dict(restore=-1, radius=0), (8, 8), "restore value -1"),
])
def test_argument_errors(kw, shape, msg):
    with pytest.raises(ValueError, match=msg):
        mq.check_mosquito_args([(16, 16), shape], **kw)
    if all(isinstance(v, int) for v in kw.values()):
        with pytest.raises(ValueError, match=msg):
            mq.mosquito_nr(np.zeros(shape, np.uint8), **kw)


def test_chroma_too_small_is_rejected_only_when_processed():
    planes = [np.zeros((6, 6), np.uint8), np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.uint8)]
    with pytest.raises(ValueError, match="too small"):
        mq.mosquito_frame(planes, which=(0, 1, 2))
    assert len(mq.mosquito_frame(planes)) == 3


def test_smallest_plane_and_bounds_are_accepted():
    a = fx.splitmix64_plane(3, (4, 4), np.uint8)
    for st, rs, rd in ((0, 0, 1), (32, 128, 2), (32, 0, 1), (1, 1, 2)):
        assert mq.mosquito_nr(a, st, rs, rd).shape == (4, 4)


# ---- conditions on the inputs the GPU suites reuse ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bits", [(np.uint8, 8), (np.uint16, 16), (np.float32, 32)], ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("radius", [1, 2])
def test_noise_reaches_all_nine_direction_classes(dtype, bits, radius):
    a = fx.splitmix64_plane(7, (48, 64), dtype)
    if np.dtype(dtype) != np.float32:
        a = (a >> (bits - 3)).astype(dtype)  # eight levels: ties and flat samples among random directions
    else:
        a = (np.floor(a * 8) / 8).astype(np.float32)
    m = mq.intermediates(a, 16, 128, radius, None if bits == 32 else bits)
    assert set(np.unique(m["dir"]).tolist()) == set(range(9))
    full = mq.intermediates(fx.splitmix64_plane(8, (48, 64), dtype), 16, 128, radius)
    assert set(range(8)) <= set(np.unique(full["dir"]).tolist())


@pytest.mark.parametrize("dtype,bits", [(np.uint8, 8), (np.uint16, 10), (np.uint16, 16), (np.float32, 32)], ids=["u8", "u10", "u16", "f32"])
def test_binary_noise_reaches_both_clamps(dtype, bits):
    a = binary_noise(5, (64, 66), dtype, bits)
    m = mq.intermediates(a, 32, 128, 2, None if bits == 32 else bits)
    peak = 1.0 if bits == 32 else (1 << bits) - 1
    assert m["pre"].min() < 0 and m["pre"].max() > peak
    out = mq.mosquito_nr(a, 32, 128, 2, None if bits == 32 else bits)
    assert out.min() == 0 and out.max() == peak


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("restore", [0, 1, 64, 127, 128])
def test_16_bit_wrapping_and_32_bit_agree_for_8_bit_input(radius, restore):
    for strength in (1, 16, 32):
        for a in (binary_noise(11, (33, 40), np.uint8, 8), fx.splitmix64_plane(12, (33, 40), np.uint8)):
            x, y = mq.intermediates(a, strength, restore, radius, work=16), mq.intermediates(a, strength, restore, radius, work=32)
            assert all(np.array_equal(x[k], y[k]) for k in ("dir", "blur", "pre"))


def test_intermediates_are_consistent_with_the_output():
    a = fx.splitmix64_plane(21, (20, 30), np.uint16)
    m = mq.intermediates(a, 16, 0, 2, 16)
    assert np.array_equal(m["pre"], (m["blur"] + 8) >> 4)  # restore = 0: the smoothing alone
    assert np.array_equal(mq.mosquito_nr(a, 16, 0, 2, 16), np.clip(m["pre"], 0, 65535))
    flat = mq.intermediates(np.full((9, 9), 100, np.uint8), 32, 128, 2)
    assert (flat["dir"] == 8).all() and (flat["pre"] == 100).all()


def test_library_exports_the_entry_point():
    from vszip_amd import capi

    lib = ctypes.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "vszip_mosquito_nr")
    assert "vszip_mosquito_nr" in capi.SYMBOLS and len(capi.SYMBOLS["vszip_mosquito_nr"][1]) == 9
    assert capi.load().vszip_abi_version() == 4
    assert all(hasattr(capi.Device, n) for n in ("mosquito_nr", "prepared_mosquito_nr"))
