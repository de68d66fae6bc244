"""CPU: the Deband parity spec (tests/deband_ref.py) reproduces the reference's tests/goldens/deband.json
(tests/golden/deband_goldens.json) from tests/fixtures.py's inputs, restates the behavioural tests and the numeric known
answers of the reference's tests/test_deband.py, raises the wrapper's errors with its wording, and the library's device-free
table generator (vszip_deband_tables, through ctypes) equals the spec's tables byte for byte.

The file holds 43 keys with 63 planes; 40 keys are rebuilt (deband_ref.LEFT_OUT names the three 8-bit keys, which pass
through the host's resizer before and after the filter)."""
import ctypes

import numpy as np
import pytest

import deband_ref as db
import fixtures as fx

KEYS = sorted(db.goldens())
RUN = [k for k in KEYS if k not in db.LEFT_OUT]


def test_all_43_keys_are_committed_and_what_is_left_out_is_listed():
    assert len(KEYS) == 43 and sum(len(v) for v in db.goldens().values()) == 63
    assert set(db.LEFT_OUT) <= set(KEYS) and len(db.LEFT_OUT) <= 4
    assert sorted(set(KEYS) - set(RUN)) == sorted(db.LEFT_OUT)
    assert {db.parse_key(k)[0] for k in db.LEFT_OUT} == {"GRAY8", "YUV420P8", "YUV422P8"}  # RGB48 is rebuilt (RGB24 x 257)
    assert {db.parse_key(k)[1] for k in KEYS} == {"full", "odd", "tiny"}


def test_parse_key():
    assert db.parse_key("GRAY16|tiny|grain=16,seed=7,thr=48") == ("GRAY16", "tiny", dict(grain=16, seed=7, thr=48))
    assert db.parse_key("YUV444PS|full|grain=[16,8],seed=7,thr=[48,24,12]")[2] == dict(grain=[16, 8], seed=7, thr=[48, 24, 12])
    assert db.parse_key("GRAY16|full|grain=16,max_angle=0.5,sample_mode=7,seed=7,thr=48")[2]["max_angle"] == 0.5
    assert db.parse_key("GRAY16|full|blur_first=0,grain=16,seed=7,thr=48")[2]["blur_first"] is False


def _check(key, outs):
    want = db.goldens()[key]
    assert len(outs) == len(want)
    for i, o in enumerate(outs):
        st, g = fx.plane_stats(o), want[f"p{i}"]
        if o.dtype.kind == "f":
            assert st["min"] == pytest.approx(g["min"], abs=1e-7, rel=0) and st["max"] == pytest.approx(g["max"], abs=1e-7, rel=0), (key, i, st, g)
        else:
            assert st["min"] == g["min"] and st["max"] == g["max"], (key, i, st, g)
        assert st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i, st, g)


@pytest.mark.parametrize("key", RUN)
def test_restatement_reproduces_golden(key):
    _check(key, db.run_key(key))


@pytest.mark.parametrize("key", [k for k in RUN if "|tiny|" in k])
def test_tiny_keys_need_32_byte_frame_alignment(key):
    """the grain index is y * pitch + x with VapourSynth's row pitch: 13 samples of 16 bits have a 16-sample pitch under 32-byte
    alignment and a 32-sample pitch under 64-byte alignment; only the former reproduces the golden"""
    _check(key, db.run_key(key, align=32))
    other = db.run_key(key, align=64)
    assert not np.array_equal(other[0], db.run_key(key, align=32)[0])
    with pytest.raises(AssertionError):
        _check(key, other)


# ---- the table generator of the library --------------------------------------------------------------------------------------
def _same_tables(a, b):
    for k in ("luma", "chroma", "grain_y", "grain_c", "grain_offsets"):
        x, y = a[k], b[k]
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert a["max_offset"] == b["max_offset"] and a["items"] == b["items"]


def _table_cases():
    n = 0
    for (w, h) in [(13, 7), (203, 45)]:
        for algo in [(1, 1), (0, 0), (2, 2), (0, 2), (2, 1)]:
            for mode in (1, 2, 3, 4):
                for ss in [(0, 0), (1, 1), (1, 0)]:
                    for rng in (0, 1, 15, 31, 255):
                        n += 1
                        if w > 100 and n % 6:  # the larger plane: a sixth of the grid, still every generator, mode, subsampling and range
                            continue
                        fl = bool(n % 2)
                        yield dict(width=w, height=h, ssw=ss[0], ssh=ss[1], num_frames=3, range=rng, sample_mode=mode, seed=7 * n - 900,
                                   random_algo_ref=algo[0], random_algo_grain=algo[1], random_param_ref=1.5, random_param_grain=2.0,
                                   grain=((0.0627, 0.03) if fl else (4112, 0)) if n % 5 else ((0.0, 0.01) if fl else (0, 2056)), dynamic_grain=n % 3 == 0, is_float=fl)


def test_library_table_generator_equals_the_spec():
    from vszip_amd import capi

    seen = set()
    for kw in _table_cases():
        _same_tables(capi.deband_tables(**kw), db.tables(**kw))
        seen.add((kw["random_algo_ref"], kw["random_algo_grain"], kw["sample_mode"], kw["ssw"], kw["ssh"], kw["range"], kw["width"], kw["dynamic_grain"]))
    assert len(seen) == 350  # 300 at 13 x 7 (5 generator pairs x 4 modes x 3 subsamplings x 5 ranges), every sixth of them at 203 x 45
    for algo in (0, 1, 2):
        for w in (13, 203):
            assert any(s[0] == algo and s[6] == w and s[7] for s in seen) and any(s[1] == algo and s[6] == w for s in seen)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_library_table_generator_at_range_255_with_wrapped_entries(mode):
    """300 x 280 at range 255: cur_range reaches 128 and more in the middle, where a random value of +-128 wraps to -128"""
    from vszip_amd import capi

    kw = dict(width=300, height=280, ssw=1, ssh=1, num_frames=3, range=255, sample_mode=mode, seed=0, grain=(4112, 2056), dynamic_grain=True)
    a, b = capi.deband_tables(**kw), db.tables(**kw)
    assert (b["luma"] == -128).any() and b["max_offset"] == 128
    _same_tables(a, b)


def test_fast_and_serial_builders_of_the_spec_agree():
    kw = dict(width=29, height=17, ssw=1, ssh=1, num_frames=3, range=15, sample_mode=2, seed=7, grain=(4112, 2056), dynamic_grain=True)
    _same_tables(db.tables(fast=True, **kw), db.tables(fast=False, **kw))
    for algo in (0, 1, 2):
        r1, r2 = db.Rng(12345), db.Rng(12345)
        assert np.array_equal(db.bulk_reals(r1, algo, 2.0, 3000), np.array([r2.real(algo, 2.0) for _ in range(3000)])) and r1.s == r2.s


def test_chroma_table_is_the_luma_table_at_the_chroma_sites():
    t = db.tables(26, 14, 1, 0, range=5, sample_mode=2, seed=3)
    assert np.array_equal(t["chroma"], t["luma"][:, ::2]) and t["chroma"].shape == (14, 13, 2)
    assert (np.abs(t["luma"].astype(int)) <= 5).all() and t["max_offset"] == 5
    assert not t["luma"][0].any() and not t["luma"][:, 0].any()  # no room at the edges
    assert not db.tables(26, 14, range=5, sample_mode=4)["luma"][..., 1].any()  # val2 only in mode 2


# ---- the create-time checks ------------------------------------------------------------------------------------------------
ERRORS = [
    (dict(sample_mode=8), r'parameter "sample_mode=8" out of range \[1\.\.7\]'),
    (dict(range=256), r'parameter "range=256" out of range \[0\.\.255\]'),
    (dict(max_angle=2.0), r'parameter "max_angle=2" out of range \[0\.\.1\]'),
    (dict(thr=[1, 2, 3, 4]), r'parameter "thr" has too many elements \(got 4, max 3\)'),
    (dict(grain=[1, 2, 3]), r'parameter "grain" has too many elements \(got 3, max 2\)'),
    (dict(thr=[300]), r'parameter "thr\[0\]=300" out of range \[0\.\.255\]'),
    (dict(grain=200), r'parameter "grain\[0\]=200" out of range \[0\.\.127\]'),
    (dict(thr1=[1, 2, 3, 4]), r'parameter "thr1" has too many elements \(got 4, max 3\)'),
    (dict(thr1=[300]), r'parameter "thr1\[0\]=300" out of range \[0\.\.255\]'),
    (dict(thr2=[1, 2, 3, 4]), r'parameter "thr2" has too many elements \(got 4, max 3\)'),
    (dict(thr2=[300]), r'parameter "thr2\[0\]=300" out of range \[0\.\.255\]'),
    (dict(thr=[-1]), r'parameter "thr\[0\]=-1" out of range \[0\.\.255\]'),
    (dict(grain=[-1]), r'parameter "grain\[0\]=-1" out of range \[0\.\.127\]'),
    (dict(sample_mode=0), r'parameter "sample_mode=0" out of range \[1\.\.7\]'),
    (dict(range=-1), r'parameter "range=-1" out of range \[0\.\.255\]'),
    (dict(random_algo_ref=3), r'parameter "random_algo_ref=3" out of range \[0\.\.2\]'),
    (dict(random_algo_ref=-1), r'parameter "random_algo_ref=-1" out of range \[0\.\.2\]'),
    (dict(random_algo_grain=3), r'parameter "random_algo_grain=3" out of range \[0\.\.2\]'),
    (dict(random_param_ref=256), r'parameter "random_param_ref=256" out of range \[0\.\.255\]'),
    (dict(random_param_ref=-1), r'parameter "random_param_ref=-1" out of range \[0\.\.255\]'),
    (dict(random_param_grain=256), r'parameter "random_param_grain=256" out of range \[0\.\.255\]'),
    (dict(max_angle=-0.5), r'parameter "max_angle=-0.5" out of range \[0\.\.1\]'),
    (dict(angle_boost=-1.0), r'parameter "angle_boost=-1" out of range \[0\.\.65535\]'),
    (dict(angle_boost=70000.0), r'parameter "angle_boost=70000" out of range \[0\.\.65535\]'),
    (dict(random_param_grain=-1), r'parameter "random_param_grain=-1" out of range \[0\.\.255\]'),
    (dict(random_algo_grain=-1), r'parameter "random_algo_grain=-1" out of range \[0\.\.2\]'),
]
TABLE_KEYS = ("sample_mode", "range", "random_algo_ref", "random_algo_grain", "random_param_ref", "random_param_grain")


@pytest.mark.parametrize("kw,msg", ERRORS, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in ERRORS])
def test_argument_errors(kw, msg):
    with pytest.raises(ValueError, match="Deband: " + msg + r"\."):
        db.check_args(**kw)
    if set(kw) <= set(TABLE_KEYS):  # what the table generator is given, it checks itself, with the same words
        from vszip_amd import capi

        with pytest.raises(ValueError, match="Deband: " + msg + r"\."):
            capi.deband_tables(16, 16, **kw)


def test_order_of_the_checks():
    with pytest.raises(ValueError, match='"thr'):
        db.check_args(thr=[300], grain=200, sample_mode=9)
    with pytest.raises(ValueError, match='"grain'):
        db.check_args(grain=200, sample_mode=9)
    with pytest.raises(ValueError, match="sample_mode"):
        db.check_args(sample_mode=9, range=300)
    from vszip_amd import capi

    with pytest.raises(ValueError, match="sample_mode"):
        capi.deband_tables(16, 16, sample_mode=9, range=300, random_algo_ref=5)
    with pytest.raises(ValueError, match='"range=300"'):
        capi.deband_tables(16, 16, range=300, random_algo_ref=5)


def test_short_arrays_repeat_the_last_value_and_thr1_thr2_default_to_thr():
    a = db.check_args(thr=[48, 24], grain=[16, 8])
    assert a["thr"] == [48, 24, 24] and a["thr1"] == a["thr"] and a["thr2"] == a["thr"] and a["grain"] == [16, 8, 8]
    assert db.scale_value([48, 0.99, 127], False) == [12336, 254, 32639]
    assert db.check_args(dynamic_grain=True)["dynamic_grain"] is False  # no grain: nothing to move


# ---- the reference's behavioural tests and known answers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def banded16():
    return db.banded16()


@pytest.fixture(scope="module")
def banded_f32(banded16):
    from oracle import vs_host as vh

    return vh.int_to_float(banded16, 16, True)


def avg(p):
    return fx.plane_stats(p)["avg"]


@pytest.mark.parametrize("mode", range(1, 8))
def test_passthrough_when_disabled(banded16, banded_f32, mode):
    assert np.array_equal(db.deband_frame([banded16], thr=0, grain=0, sample_mode=mode)[0], banded16)
    assert np.array_equal(db.deband_frame([banded_f32], thr=0, grain=0, sample_mode=mode)[0], banded_f32)


def test_deterministic(banded16):
    a, b = (db.deband_frame([banded16], thr=48, grain=32, seed=7)[0] for _ in range(2))
    assert np.array_equal(a, b)
    assert not np.array_equal(a, db.deband_frame([banded16], thr=48, grain=32, seed=8)[0])


SAMPLE_MODE_GOLDENS = {1: 0.48633140688181886, 2: 0.4862626649881743, 3: 0.4869006446936751, 4: 0.48657496471351186, 5: 0.48692404345006485,
                       6: 0.4868622815903477, 7: 0.4868109427303874}


@pytest.mark.parametrize("mode", range(1, 8))
def test_sample_modes_known_answers(banded16, mode):
    """the reference's tolerance (rel 1e-6); modes 1 to 5 come out to the last digit"""
    out = db.deband_frame([banded16], thr=48, sample_mode=mode, seed=7)[0]
    assert avg(out) == pytest.approx(SAMPLE_MODE_GOLDENS[mode], rel=1e-6)
    if mode <= 5:
        assert avg(out) == pytest.approx(SAMPLE_MODE_GOLDENS[mode], rel=1e-12)
    assert not np.array_equal(out, banded16)


def test_float_known_answer(banded_f32):
    assert avg(db.deband_frame([banded_f32], thr=48, sample_mode=2, seed=7)[0]) == pytest.approx(0.4955954249984279, rel=1e-6)


def test_grain_known_answer(banded16):
    out = db.deband_frame([banded16], thr=0, grain=64, seed=7)[0]
    assert avg(out) == pytest.approx(0.48693080666878863, rel=1e-6) and not np.array_equal(out, banded16)


def test_dynamic_and_static_grain_across_two_frames(banded16):
    run = lambda n, dyn: db.deband_frame([banded16], n=n, num_frames=2, thr=0, grain=64, seed=7, dynamic_grain=dyn)[0]
    assert np.array_equal(run(0, False), run(1, False))
    assert not np.array_equal(run(0, True), run(1, True))


def _blank(shape, dtype, values):
    return [np.full(shape if i == 0 else (shape[0] >> 1, shape[1] >> 1), v, dtype) for i, v in enumerate(values)]


def test_keep_tv_range_clamps_yuv_to_60160_and_61440():
    hi, lo = _blank((32, 64), np.uint16, [65000, 64000, 63000]), _blank((32, 64), np.uint16, [64500, 63500, 62500])
    src = [np.vstack([a, b]) for a, b in zip(hi, lo)]
    clamped = db.deband_frame(src, "YUV", 1, 1, thr=48, seed=7, keep_tv_range=True)
    assert [int(p.max()) for p in clamped] == [60160, 61440, 61440]
    assert db.deband_frame(src, "YUV", 1, 1, thr=48, seed=7, keep_tv_range=False)[0].max() > 60160


@pytest.mark.parametrize("family,values", [("YUV", [1.0, 0.0, 0.0]), ("GRAY", [1.0]), ("RGB", [1.0, 1.0, 1.0])])
def test_keep_tv_range_is_inert_on_float_and_rgb(family, values):
    src = [np.full((32, 64), v, np.float32) for v in values]
    on = db.deband_frame(src, family, thr=48, grain=64, seed=7, keep_tv_range=True)
    off = db.deband_frame(src, family, thr=48, grain=64, seed=7, keep_tv_range=False)
    assert all(np.array_equal(a, b) for a, b in zip(on, off))
    rgb = [np.full((32, 64), 65000, np.uint16)] * 3
    assert all(np.array_equal(a, b) for a, b in zip(db.deband_frame(rgb, "RGB", thr=48, grain=64, seed=7, keep_tv_range=True),
                                                    db.deband_frame(rgb, "RGB", thr=48, grain=64, seed=7)))


def test_float_is_clamped_to_full_range():
    src = [np.vstack([np.full((32, 64), a, np.float32), np.full((32, 64), b, np.float32)]) for a, b in ((1.0, 0.0), (0.5, -0.5), (0.5, -0.5))]
    y, u, v = db.deband_frame(src, "YUV", thr=48, grain=96, seed=7)
    assert y.min() == 0.0 and y.max() == 1.0
    assert u.min() == -0.5 and u.max() == 0.5 and v.min() == -0.5 and v.max() == 0.5
    for p in db.deband_frame([src[0]] * 3, "RGB", thr=48, grain=96, seed=7):
        assert p.min() == 0.0 and p.max() == 1.0


def test_random_algos_differ(banded16):
    outs = [db.deband_frame([banded16[:64, :96]], thr=48, grain=32, seed=7, random_algo_ref=a, random_algo_grain=a)[0] for a in (0, 1, 2)]
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])


def test_grain_at_limit():
    src = np.full((64, 64), 32768, np.uint16)
    assert not np.array_equal(db.deband_frame([src], thr=0, grain=127, seed=7)[0], src)


def test_mode_7_boost_is_taken_for_some_samples_and_not_for_others():
    src = db.golden_inputs("GRAY16", "full")[0]
    m = db.boost_mask(src, db.tables(src.shape[1], src.shape[0], sample_mode=7, seed=7)["luma"], 0, 0, 0.15)
    assert 0.05 < m.mean() < 0.95


def test_library_exports_the_entry_points():
    from vszip_amd import capi

    lib = ctypes.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "vszip_deband") and hasattr(lib, "vszip_deband_tables")
    assert len(capi.SYMBOLS["vszip_deband"][1]) == 10 and len(capi.SYMBOLS["vszip_deband_tables"][1]) == 10
    assert capi.load().vszip_abi_version() == 4
    assert all(hasattr(capi.Device, n) for n in ("deband", "prepared_deband", "deband_entry", "upload_deband_tables")) and hasattr(capi, "deband_tables")
    assert ctypes.sizeof(capi.DebandPlane) == 64 and ctypes.sizeof(capi.DebandCfg) == 80
