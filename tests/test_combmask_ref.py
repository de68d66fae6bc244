"""CPU: the CombMask / CombMaskMT parity spec (tests/combmask_ref.py) reproduces every key of the reference's
tests/goldens/combmask.json (tests/golden/combmask_goldens.json) and the numbers hard-coded in the reference's
tests/test_combmask.py from tests/fixtures.py's inputs, and libvszip_hip.so exports the two entry points."""
import ctypes

import numpy as np
import pytest

import combmask_ref as cr
import fixtures as fx

KEYS = sorted(cr.goldens())


def _avg(a):
    return fx.plane_stats(a)["avg"]


def test_all_39_keys_are_committed():
    assert len(KEYS) == 39
    filts = [cr.parse_key(k)[2] for k in KEYS]
    assert filts.count("CombMask") == 21 and filts.count("CombMaskMT") == 18
    assert {cr.parse_key(k)[0] for k in KEYS} == {"GRAY8", "YUV420P8", "YUV444P8"}
    # the eight (metric, expand, motion) variants and both MT forms are among them
    variants = {(kw.get("metric", 0), kw.get("expand", True), kw.get("mthresh", 9) > 0) for _, _, f, kw in map(cr.parse_key, KEYS) if f == "CombMask"}
    assert len(variants) == 8
    assert {kw.get("thy1", 30) == kw.get("thy2", 30) for _, _, f, kw in map(cr.parse_key, KEYS) if f == "CombMaskMT"} == {True, False}


@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_golden(key):
    want = cr.goldens()[key]
    outs = cr.run_key(key)
    assert len(outs) == len(want)
    for i, o in enumerate(outs):
        st, g = fx.plane_stats(o), want[f"p{i}"]
        assert st["min"] == g["min"] and st["max"] == g["max"], (key, i, st, g)
        assert st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i)


@pytest.fixture(scope="module")
def src8():
    """frames 0 and 1 of the reference's src8: the temporal clip as GRAY8 through a point resize"""
    return fx.luma8(fx.temporal_rgb24(0)), fx.luma8(fx.temporal_rgb24(1))


# reference tests/test_combmask.py GOLDENS: frame-1 averages
@pytest.mark.parametrize("args,expected", [
    (dict(), 0.206181640625),
    (dict(cthresh=8, mthresh=2, metric=0), 0.1980615234375),
    (dict(cthresh=8, mthresh=2, metric=1), 0.2363623046875),
    (dict(cthresh=8, mthresh=100), 0.05046875),
    (dict(cthresh=8, mthresh=2, expand=False), 0.094482421875),
])
def test_reference_frame1_averages(src8, args, expected):
    f0, f1 = src8
    assert _avg(cr.comb_mask(f1, f0, **args)) == pytest.approx(expected, rel=1e-9, abs=0)


def test_first_frame_has_no_motion(src8):
    f0, _ = src8
    assert _avg(cr.comb_mask(f0, f0, cthresh=8, mthresh=2)) == 0.0
    assert _avg(cr.comb_mask(f0, f0, cthresh=8, mthresh=0)) == pytest.approx(0.196611328125, rel=1e-9, abs=0)
    assert _avg(cr.comb_mask(f0, None, cthresh=8, mthresh=0)) == pytest.approx(0.196611328125, rel=1e-9, abs=0)


def test_mt_reference_averages():
    g = fx.crop_gray8()
    assert _avg(cr.comb_mask_mt(g)) == pytest.approx(0.1150439453125, rel=1e-9, abs=0)
    assert _avg(cr.comb_mask_mt(g, 0, 255)) == pytest.approx(0.10427868412990196, rel=1e-9, abs=0)


def test_output_is_binary(src8):
    f0, f1 = src8
    for kw in (dict(metric=0), dict(metric=1), dict(expand=False)):
        assert set(np.unique(cr.comb_mask(f1, f0, **kw))) <= {0, 255}
    assert set(np.unique(cr.comb_mask_mt(fx.crop_gray8()))) <= {0, 255}


def test_expand_is_superset(src8):
    f0, f1 = src8
    for metric in (0, 1):
        expanded = cr.comb_mask(f1, f0, cthresh=8, mthresh=0, metric=metric)
        plain = cr.comb_mask(f1, f0, cthresh=8, mthresh=0, expand=False, metric=metric)
        assert (expanded >= plain).all() and (expanded != plain).any()
        assert np.array_equal(expanded[:, -1], plain[:, -1])  # column w - 1 is never expanded


def test_mt_gradient_has_intermediate_values():
    out = cr.comb_mask_mt(fx.crop_gray8(), 0, 255)
    assert ((out > 0) & (out < 255)).any()
    assert not out[0].any() and not out[-1].any()


def test_metric1_allows_large_cthresh(src8):
    f0, f1 = src8
    assert _avg(cr.comb_mask(f1, f0, cthresh=300, metric=1)) > 0.0


def test_motion_dilation_at_the_edge_rows():
    """motion in row 0 only reaches rows 0 and 1; motion in row h - 1 only reaches rows h - 2 and h - 1"""
    s = np.zeros((8, 9), np.uint8)
    s[::2] = 200  # combed everywhere
    for row, reached in ((0, [0, 1]), (7, [6, 7])):
        p = s.copy()
        p[row] ^= 0x80
        out = cr.comb_mask(s, p, cthresh=6, mthresh=9, expand=False)
        assert sorted(set(np.nonzero(out)[0])) == reached


def test_small_widths_are_not_expanded():
    s = np.array([[0], [255], [0], [255]], np.uint8)
    assert np.array_equal(cr.comb_mask(s, None, 6, 0, True), cr.comb_mask(s, None, 6, 0, False))
    s2 = np.array([[0, 0], [255, 0], [0, 0]], np.uint8)
    out = cr.comb_mask(s2, None, 6, 0, True)
    assert out[:, 0].all() and not out[:, 1].any()  # column 0 = m0 | m1; column w - 1 keeps its own


@pytest.mark.parametrize("call,msg", [
    (lambda a: cr.comb_mask(a, None, cthresh=256, mthresh=0), "cthresh must be between 0 and 255 when metric = false"),
    (lambda a: cr.comb_mask(a, None, cthresh=-1, mthresh=0), "cthresh must be between 0 and 255 when metric = false"),
    (lambda a: cr.comb_mask(a, None, cthresh=65026, mthresh=0, metric=1), "cthresh must be between 0 and 65025 when metric = true"),
    (lambda a: cr.comb_mask(a, a, mthresh=256), "mthresh must be between 0 and 255"),
    (lambda a: cr.comb_mask(a, a, mthresh=-1), "mthresh must be between 0 and 255"),
    (lambda a: cr.comb_mask(a[:2], a[:2]), "clip too small; every plane must be at least 3 rows tall"),
    (lambda a: cr.comb_mask_mt(a, -1, 30), r"thY1 value should be in range \[0;255\]"),
    (lambda a: cr.comb_mask_mt(a, 30, 256), r"thY2 value should be in range \[0;255\]"),
    (lambda a: cr.comb_mask_mt(a, 31, 30), "thY1 can't be greater than thY2"),
    (lambda a: cr.comb_mask_mt(a[:2]), "clip too small; every plane must be at least 3 rows tall"),
])
def test_argument_errors(call, msg):
    with pytest.raises(ValueError, match=msg):
        call(np.zeros((4, 8), np.uint8))


def test_library_exports_the_entry_points():
    from vszip_amd import capi

    lib = ctypes.CDLL(str(capi.LIB_PATH))
    for name in ("vszip_comb_mask", "vszip_comb_mask_mt"):
        assert hasattr(lib, name)
        assert name in capi.SYMBOLS
    assert capi.load().vszip_abi_version() == 4
    assert hasattr(capi.Device, "comb_mask") and hasattr(capi.Device, "comb_mask_mt") and hasattr(capi.Device, "prepared_comb_mask")
