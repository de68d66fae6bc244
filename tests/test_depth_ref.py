"""CPU: the depth-conversion spec (tests/depth_ref.py). Up to 16 bits, deband_ref.deband_frame, error-diffusion dither back rebuilds the
three 8-bit keys of the reference's Deband goldens that deband_ref.LEFT_OUT leaves out, with the criterion those goldens allow (min and
max equal, |avg - golden| * w * h * peak < 0.5: the sum of all samples is equal). The serial and the anti-diagonal builder agree;
`none` restates the rule deband_ref.banded16 states; the library's device-free argument check (vszip_depth_check, what vszip_depth
runs first) gives the spec's codes and texts."""
import numpy as np
import pytest

import deband_ref as db
import depth_ref as dr
import fixtures as fx


def test_the_left_out_keys_are_the_8_bit_ones():
    assert sorted(db.LEFT_OUT) == sorted(["GRAY8|full|grain=16,seed=7,thr=48", "YUV420P8|full|grain=16,seed=7,thr=48", "YUV422P8|full|grain=[16,8],seed=7,thr=[48,24]"])


@pytest.mark.parametrize("key", sorted(db.LEFT_OUT))
def test_spec_rebuilds_the_8_bit_goldens(key):
    outs = dr.run_key8(key)
    assert len(outs) == len(db.goldens()[key]) and all(o.dtype == np.uint8 for o in outs)
    for i, o in enumerate(outs):
        print(key, i, fx.plane_stats(o), db.goldens()[key][f"p{i}"])
    assert dr.same_as_golden(key, outs) == []


def test_the_criterion_sees_one_count():
    """a single sample one count off moves avg by 1 / (w h peak): outside the bound"""
    key = "GRAY8|full|grain=16,seed=7,thr=48"
    outs = [o.copy() for o in dr.run_key8(key)]
    y, x = np.argwhere((outs[0] > outs[0].min()) & (outs[0] < outs[0].max() - 1))[0]
    outs[0][y, x] += 1
    assert [b[0] for b in dr.same_as_golden(key, outs)] == [0]


_content = dr.content


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (7, 1), (13, 7), (65, 66), (130, 131)])
def test_serial_and_fast_builders_agree(h, w):
    for bits_in, bits_out, full in ((16, 8, False), (16, 10, False), (10, 8, False), (16, 8, True), (12, 15, True)):
        a = _content(h * 1000 + w + bits_out, h, w, bits_in)
        fast, serial = (dr.convert(a, bits_in, bits_out, dr.ERROR_DIFFUSION, full, fast=f) for f in (True, False))
        assert fast.dtype == dr.dtype_of(bits_out) and np.array_equal(fast, serial), (h, w, bits_in, bits_out, full)


def test_error_diffusion_keeps_the_mean_and_differs_from_rounding():
    a = _content(5, 65, 66, 16)
    none, ed = dr.convert(a, 16, 8, dr.NONE), dr.convert(a, 16, 8, dr.ERROR_DIFFUSION)
    # a sample changes when the incoming error carries its fraction across .5: errors uniform in [-.5, .5] weighted 7, 3, 5, 1 sixteenths sum to a
    # standard deviation of 0.29 * sqrt(84) / 16 = 0.17, a mean magnitude of 0.13; 5 of 7 samples are noise (the rest hold at 0 or the peak): 0.09
    assert (none != ed).mean() > 0.045
    inner = (a > 1024) & (a < 64000)  # away from the clamp the diffused error keeps the local mean
    assert abs(ed[inner].astype(np.float64).mean() - a[inner].astype(np.float64).mean() / 256) < 0.05


def test_none_down_is_the_rule_banded16_states():
    g = fx.crop_gray16()
    g8 = dr.convert(g, 16, 8, dr.NONE)
    assert np.array_equal(g8, np.clip(np.rint(g.astype(np.float32) * np.float32(1.0 / 256.0)), 0, 255).astype(np.uint8))
    assert np.array_equal(dr.convert(g8, 8, 16, dr.NONE), db.banded16())
    ties = np.array([[128, 384, 640, 65535, 65408, 0]], np.uint16)  # x.5 goes to even; the top clamps
    assert dr.convert(ties, 16, 8, dr.NONE).tolist() == [[0, 2, 2, 255, 255, 0]]


def test_none_up_is_the_shift_and_full_range_8_to_16_is_times_257():
    a8 = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(dr.convert(a8, 8, 16, dr.NONE), a8.astype(np.uint16) << 8)
    assert np.array_equal(dr.convert(a8, 8, 10, dr.NONE), a8.astype(np.uint16) << 2)
    assert np.array_equal(dr.convert(a8, 8, 16, dr.NONE, full_range=True), a8.astype(np.uint16) * np.uint16(257))
    a10 = np.arange(1024, dtype=np.uint16).reshape(32, 32)
    assert np.array_equal(dr.convert(a10, 10, 15, dr.NONE), a10 << 5)
    assert np.array_equal(dr.convert(a10, 10, 10, dr.ERROR_DIFFUSION), a10)  # scale 1: no error to diffuse
    assert dr.scale_of(16, 8, True) == np.float32(255.0 / 65535.0) and dr.scale_of(16, 8) == np.float32(1 / 256)


OK = (1, 1, 8, 8, 8, 8, 0)  # src, dst (non-NULL), w, h, pitches, chroma
ERRORS = [
    (dict(bits_in=7), dr.ERR_ARG, "Depth: bits_in 7 is outside 8..16"),
    (dict(bits_in=17), dr.ERR_ARG, "Depth: bits_in 17 is outside 8..16"),
    (dict(bits_out=32), dr.ERR_ARG, "Depth: bits_out 32 is outside 8..16"),
    (dict(dither=2), dr.ERR_ARG, "Depth: dither 2 is neither 0 (none) nor 1 (error diffusion)"),
    (dict(dither=-1), dr.ERR_ARG, "Depth: dither -1 is neither 0 (none) nor 1 (error diffusion)"),
    (dict(planes=[]), dr.ERR_ARG, "Depth: no planes"),
    (dict(planes=[OK, (0, 1, 8, 8, 8, 8, 0)]), dr.ERR_ARG, "Depth: plane 1: src and dst must not be NULL"),
    (dict(planes=[(1, 0, 8, 8, 8, 8, 0)]), dr.ERR_ARG, "Depth: plane 0: src and dst must not be NULL"),
    (dict(planes=[OK, OK, (1, 1, 0, 8, 8, 8, 0)]), dr.ERR_ARG, "Depth: plane 2: bad geometry 0x8, pitches 8 -> 8"),
    (dict(planes=[(1, 1, 8, 0, 8, 8, 0)]), dr.ERR_ARG, "Depth: plane 0: bad geometry 8x0, pitches 8 -> 8"),
    (dict(planes=[(1, 1, 9, 8, 8, 16, 0)]), dr.ERR_ARG, "Depth: plane 0: bad geometry 9x8, pitches 8 -> 16"),
    (dict(planes=[(1, 1, 9, 8, 16, 8, 0)]), dr.ERR_ARG, "Depth: plane 0: bad geometry 9x8, pitches 16 -> 8"),
    (dict(full_range=1, planes=[OK, (1, 1, 8, 8, 8, 8, 1)]), dr.ERR_UNSUPPORTED, "Depth: plane 1: full-range chroma is not built (DESIGN.md section 1)"),
    # the order of the checks
    (dict(bits_in=7, bits_out=7, dither=5, planes=[]), dr.ERR_ARG, "Depth: bits_in 7 is outside 8..16"),
    (dict(bits_out=7, dither=5, planes=[]), dr.ERR_ARG, "Depth: bits_out 7 is outside 8..16"),
    (dict(full_range=1, planes=[(1, 1, 8, 8, 8, 8, 1), (0, 1, 8, 8, 8, 8, 0)]), dr.ERR_UNSUPPORTED, "Depth: plane 0: full-range chroma is not built (DESIGN.md section 1)"),
]


@pytest.mark.parametrize("kw,code,msg", ERRORS, ids=[str(i) for i in range(len(ERRORS))])
def test_argument_errors_carry_their_texts(kw, code, msg):
    """the spec and the library's device-free check (what vszip_depth runs first) agree on code and text"""
    from vszip_amd import capi

    a = dict(bits_in=16, bits_out=8, dither=1, full_range=0, planes=[OK])
    a.update(kw)
    with pytest.raises(dr.DepthError) as e:
        dr.check_args(a["bits_in"], a["bits_out"], a["dither"], a["full_range"], [(p[0], p[1], p[2], p[3], p[4], p[5], p[6]) for p in a["planes"]])
    assert (e.value.code, str(e.value)) == (code, msg)
    with pytest.raises(capi.VszipError) as e:
        capi.depth_check(a["bits_in"], a["bits_out"], a["dither"], a["full_range"], [(p[0] or None, p[4], p[1] or None, p[5], p[2], p[3], p[6]) for p in a["planes"]])
    assert (e.value.code, str(e.value)) == (code, msg)


def test_valid_arguments_pass_and_limited_range_chroma_is_served():
    from vszip_amd import capi

    for full, chroma in ((0, 0), (0, 1), (1, 0)):
        dr.check_args(16, 8, 1, full, [(1, 1, 8, 8, 8, 8, chroma)])
        capi.depth_check(16, 8, 1, full, [(1, 8, 1, 8, 8, 8, chroma)])
    with pytest.raises(dr.DepthError) as e:
        dr.convert(np.zeros((4, 4), np.uint16), 16, 8, dr.ERROR_DIFFUSION, full_range=True, chroma=True)
    assert e.value.code == dr.ERR_UNSUPPORTED
    a = np.full((4, 4), 32768, np.uint16)
    assert np.array_equal(dr.convert(a, 16, 8, dr.NONE, chroma=True), np.full((4, 4), 128, np.uint8))  # limited range: no offset, chroma or not


def test_library_exports_the_entry_points():
    from vszip_amd import capi

    lib = capi.load()
    assert all(hasattr(lib, n) for n in ("vszip_depth", "vszip_depth_check", "vszip_deband_lowbit"))
