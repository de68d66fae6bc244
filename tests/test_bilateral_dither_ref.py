"""CPU: the BilateralDither parity spec (tests/bilateral_dither_ref.py) reproduces every key of the reference's
tests/goldens/bilateral_dither.json (tests/golden/bilateral_dither_goldens.json) from tests/fixtures.py's inputs, restates the
behavioural tests of the reference's tests/test_bilateral_dither.py that need no VapourSynth core, and the library's device-free
derivation and point-list generator (vszip_bilateral_dither_derive / _points, through ctypes) give the spec's values and bytes.
The last test counts, on the spec, that the inputs of the GPU tests take every branch of the weight and of the sum_w_min floor."""
import ctypes

import numpy as np
import pytest

import bilateral_dither_ref as bd
import fixtures as fx

KEYS = sorted(bd.goldens())
F = np.float32


def test_all_23_keys_are_committed():
    assert len(KEYS) == 23 and sum(len(v) for v in bd.goldens().values()) == 43
    assert {bd.parse_key(k)[0] for k in KEYS} == set(bd._FMT)
    assert {bd.parse_key(k)[1] for k in KEYS} == {"full", "odd"}


def test_parse_key():
    assert bd.parse_key("GRAY8|full|flat=0.4,radius=8,subspl=2,thr=8,wmin=0.5") == ("GRAY8", "full", dict(flat=0.4, radius=8, subspl=2, thr=8, wmin=0.5))
    assert bd.parse_key("YUV420P8|full|radius=[8,4,4],subspl=2,thr=[8,12,12]")[2] == dict(radius=[8, 4, 4], subspl=2, thr=[8, 12, 12])
    assert bd.parse_key("YUV444PS|full|planes=[1,2],radius=6,subspl=2,thr=16")[2]["planes"] == [1, 2]


def _check(key, outs):
    want = bd.goldens()[key]
    assert len(outs) == len(want)
    for i, o in enumerate(outs):
        st, g = fx.plane_stats(o), want[f"p{i}"]
        if o.dtype.kind == "f":
            assert st["min"] == pytest.approx(g["min"], abs=1e-7, rel=0) and st["max"] == pytest.approx(g["max"], abs=1e-7, rel=0), (key, i, st, g)
        else:
            assert st["min"] == g["min"] and st["max"] == g["max"], (key, i, st, g)
        assert st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i, st, g)


@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_golden(key):
    _check(key, bd.run_key(key))


# ---- the reference's behavioural tests -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gray16():
    return bd.golden_inputs("GRAY16", "full")[0][40:136, 200:328]


def diff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


def test_higher_thr_smooths_more(gray16):
    lo, hi = bd.filter_plane(gray16, radius=8, thr=1.0, subspl=2.0), bd.filter_plane(gray16, radius=8, thr=64.0, subspl=2.0)
    assert diff(hi, gray16) > diff(lo, gray16) > 0.0


def test_ref_equal_src_matches_no_ref_and_another_ref_changes_the_output(gray16):
    plain = bd.filter_plane(gray16, radius=8, thr=8.0, subspl=2.0)
    assert np.array_equal(bd.filter_plane(gray16, ref=gray16, radius=8, thr=8.0, subspl=2.0), plain)
    other = np.ascontiguousarray(gray16[::-1])
    assert not np.array_equal(bd.filter_plane(gray16, ref=other, radius=8, thr=8.0, subspl=2.0), plain)


def test_dense_vs_subsampled_differ(gray16):
    assert not np.array_equal(bd.filter_plane(gray16, radius=8, thr=8.0, subspl=2.0), bd.filter_plane(gray16, radius=8, thr=8.0, subspl=8.0))


def test_float_chroma_stays_in_range():
    y, u, v = (p[:64, :96] for p in bd.golden_inputs("YUV444PS", "full"))
    out = bd.frame([y, u, v], 32, radius=8, thr=24.0, subspl=8.0)
    assert out[0].min() >= -1e-6 and out[0].max() <= 1.0 + 1e-6
    for p in out[1:]:
        assert p.min() >= -0.5 - 1e-6 and p.max() <= 0.5 + 1e-6


def test_per_plane_arrays():
    src = [p[:48, :64] for p in bd.golden_inputs("YUV444P16", "full")]
    scalar = bd.frame(src, 16, radius=8, thr=8.0, flat=0.4, wmin=0.5, subspl=8.0)
    array = bd.frame(src, 16, radius=[8, 8, 8], thr=[8.0, 8.0, 8.0], flat=[0.4, 0.4, 0.4], wmin=[0.5, 0.5, 0.5], subspl=[8.0, 8.0, 8.0])
    assert all(np.array_equal(a, b) for a, b in zip(scalar, array))
    perp = bd.frame(src, 16, radius=[8, 4], thr=8.0, flat=0.4, wmin=0.5, subspl=8.0)  # the last value repeats
    assert np.array_equal(perp[0], scalar[0]) and not np.array_equal(perp[1], scalar[1]) and not np.array_equal(perp[2], scalar[2])
    luma_only = bd.frame(src, 16, radius=8, thr=16.0, subspl=8.0, planes=[0])
    assert not np.array_equal(luma_only[0], src[0]) and np.array_equal(luma_only[1], src[1]) and np.array_equal(luma_only[2], src[2])


ERRORS = [
    (dict(radius=1), "radius value 1 is below minimum 2"),
    (dict(radius=16385), "radius value 16385 is above maximum 16384"),
    (dict(thr=-1.0), "thr value -1 is below minimum 0"),
    (dict(thr=70000.0), "thr value 70000 is above maximum 65535"),
    (dict(flat=-0.1), "flat value -0.1 is below minimum 0"),
    (dict(flat=1.5), "flat value 1.5 is above maximum 1"),
    (dict(wmin=-1.0), "wmin value -1 is below minimum 0"),
    (dict(subspl=5000.0), "subspl value 5000 is above maximum 4096"),
]


@pytest.mark.parametrize("kw,msg", ERRORS, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in ERRORS])
def test_argument_errors(kw, msg):
    from vszip_amd import capi

    with pytest.raises(ValueError, match="BilateralDither: " + msg + r"\."):
        bd.derive(False, 8, **dict(dict(radius=8), **kw))
    with pytest.raises(ValueError, match="BilateralDither: " + msg + r"\."):
        capi.bilateral_dither_params(False, 8, **dict(dict(radius=8), **kw))


def test_spec_errors_of_the_frame_wrapper():
    g = bd.golden_inputs("GRAY8", "full")[0]
    with pytest.raises(ValueError, match="16x16 min"):
        bd.frame([g[:15, :15]], 8)
    with pytest.raises(ValueError, match='picture size must be greater than "radius"'):
        bd.frame([g[:20, :20]], 8, radius=24)
    with pytest.raises(ValueError, match=r"radius has too many elements \(got 4, max 3\)"):
        bd.frame([g[:20, :20]], 8, radius=[8, 8, 8, 8])
    with pytest.raises(ValueError, match="flat value 1.5 is above maximum 1"):
        bd.frame([g[:20, :20]], 8, radius=4, flat=[0.4, 1.5, 0.4])


# ---- the library's derivation and generator ----------------------------------------------------------------------------------------
RADII = (2, 3, 4, 8, 12, 16, 40)
SUBSPL = (0, 4, 8, 16, 100)


def test_library_derive_and_generator_equal_the_spec():
    from vszip_amd import capi

    small = large = 0
    for r in RADII:
        for s in SUBSPL:
            pts = bd.point_lists(r, float(s))
            K = pts.shape[1]
            small += K < 32
            large += K >= 32
            got = capi.bilateral_dither_points(r, float(s))
            assert got.dtype == pts.dtype and got.shape == pts.shape and got.tobytes() == pts.tobytes(), (r, s, K)
            assert (pts[:, 0] == 0).all() and np.abs(pts.astype(int)).max() <= r - 1
            assert all(len({(int(x), int(y)) for x, y in lst}) == K for lst in pts), (r, s)
            for is_float, bits in ((False, 8), (False, 10), (False, 16), (True, 32)):
                for thr, flat, wmin in ((2.5, 0.4, 0.0), (8.0, 0.0, 0.5), (0.001, 1.0, 3.0), (24.0, 0.7, 0.1)):
                    for sub in (float(s), 2.0):
                        a, b = capi.bilateral_dither_params(is_float, bits, r, thr, flat, wmin, sub), bd.derive(is_float, bits, r, thr, flat, wmin, sub)
                        for k in ("m", "wmax", "sum_w_min"):
                            assert F(a[k]).tobytes() == F(b[k]).tobytes(), (k, r, s, is_float, bits, thr, flat, wmin, sub, a, b)
                        assert a["K"] == b["K"] == (K if sub != 2.0 else 0) and a["subsampled"] == b["subsampled"] == (sub != 2.0)
    assert small >= 10 and large >= 10  # spirals and void-and-cluster scans


def test_known_k_and_first_points():
    assert bd.points_k(16, 0.0) == 30 and bd.points_k(8, 0.0) == 14 and bd.points_k(8, 8.0) == 28 and bd.points_k(8, 4.0) == 56 and bd.points_k(40, 0.0) == 78
    assert bd.points_k(12, 16.0) == 33 and bd.points_k(2, 4096.0) == 3 and bd.points_k(16384, 4.0) == 4096
    assert [int(v) for v in bd.row_starts(4)] == [(bd.lcg(1) >> 8) % 23, (bd.lcg(bd.lcg(1)) >> 8) % 23, (bd.lcg(bd.lcg(bd.lcg(1))) >> 8) % 23,
                                                  (bd.lcg(bd.lcg(bd.lcg(bd.lcg(1)))) >> 8) % 23]


def test_vectorised_cluster_search_equals_the_scalar_loops():
    rng = np.random.RandomState(5)
    kern = bd._vnc_kernel()
    for n in (16, 19):
        mat = (rng.rand(n, n) < 0.3).astype(np.uint16)
        for color in (0, 1):
            best, at = -1.0, (0, 0)
            for y in range(n):
                for x in range(n):
                    if mat[y, x] != color:
                        continue
                    s = 0.0
                    for j in range(-4, 5):
                        for i in range(-4, 5):
                            if mat[(y + j) % n, (x + i) % n] == color:
                                s += kern[j + 4, i + 4]
                    if s > best:
                        best, at = s, (x, y)
            assert bd._find_cluster(mat, kern, color) == at


def test_library_exports_the_entry_points():
    from vszip_amd import capi

    lib = ctypes.CDLL(str(capi.LIB_PATH))
    assert all(hasattr(lib, n) for n in ("vszip_bilateral_dither", "vszip_bilateral_dither_derive", "vszip_bilateral_dither_points"))
    assert len(capi.SYMBOLS["vszip_bilateral_dither"][1]) == 6 and capi.load().vszip_abi_version() == 4
    assert all(hasattr(capi.Device, n) for n in ("bilateral_dither", "prepared_bilateral_dither", "bilateral_dither_entry", "upload_bilateral_dither_points"))
    assert ctypes.sizeof(capi.BilateralDitherPlane) == 32 and ctypes.sizeof(capi.BilateralDitherCfg) == 20


# ---- branch coverage of the inputs of tests/test_gpu_bilateral_dither.py ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_gpu_inputs_take_every_weight_class_and_both_sides_of_the_floor(dtype):
    """thr = 8, flat = 0.4, wmin = 0.1, radius = 8, dense: each weight class (zero, saturated at wmax, in between) covers at least 5 % of the
    taps, and sum_w < sum_w_min holds for between 5 % and 95 % of the samples (measured: zero 70-78 %, saturated 11-15 %, in between 10-15 %,
    floor 9-11 %)"""
    f = np.dtype(dtype) == np.float32
    d = bd.derive(f, 32 if f else 8 * np.dtype(dtype).itemsize, 8, 8.0, 0.4, 0.1, 2.0)
    for k, (h, w) in enumerate([(45, 203), (131, 97), (16, 16)]):
        classes = []
        _, _, sw = bd.accumulate(bd.noisy_plane(3 + 3 * k, h, w, dtype), 8, d["m"], d["wmax"], classes=classes)
        share = classes[0] / classes[0].sum()
        assert (share >= 0.05).all(), (dtype, h, w, share)
        floor = float((sw < d["sum_w_min"]).mean())
        assert 0.05 <= floor <= 0.95, (dtype, h, w, floor)
