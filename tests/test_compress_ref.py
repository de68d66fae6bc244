"""CPU: the Compress parity spec (tests/compress_ref.py) reproduces every key of the reference's tests/goldens/compress.json
(tests/golden/compress_goldens.json) from tests/fixtures.py's inputs, restates the behavioural tests of the reference's
tests/test_compress.py that need no VapourSynth core, and the library's device-free table generator (vszip_compress_tables,
through ctypes) gives the spec's tables and the wrapper's error texts. The last tests count, on the spec, that the inputs of the
GPU tests take every branch of the pipeline, for both codecs."""
import ctypes

import numpy as np
import pytest

import compress_ref as cr
import fixtures as fx

KEYS = sorted(cr.goldens())


def test_all_25_keys_are_committed():
    assert len(KEYS) == 25 and sum(len(v) for v in cr.goldens().values()) == 43
    assert {cr.parse_key(k)[0] for k in KEYS} == set(cr._FMT)
    assert {cr.parse_key(k)[1] for k in KEYS} == {"full", "odd", "tiny"}
    assert {cr.parse_key(k)[2]["codec"] for k in KEYS} == {0, 1}


def test_parse_key():
    assert cr.parse_key("GRAY8|full|codec=0,dc_prec=1,qscale=8") == ("GRAY8", "full", dict(codec=0, dc_prec=1, qscale=8))
    assert cr.parse_key("YUV420P8|full|chroma=0,codec=1,quality=25")[2] == dict(chroma=False, codec=1, quality=25)


def test_golden_input_geometries():
    assert cr.golden_inputs("GRAY8", "full")[0].shape == (320, 640) and cr.golden_inputs("GRAY8", "odd")[0].shape == (319, 639)
    assert cr.golden_inputs("GRAY8", "tiny")[0].shape == (7, 13)
    assert [p.shape for p in cr.golden_inputs("YUV420P8", "full")] == [(320, 640), (160, 320), (160, 320)]
    assert [p.shape for p in cr.golden_inputs("YUV422P8", "full")] == [(320, 640), (320, 320), (320, 320)]


@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_golden(key):
    outs, want = cr.run_key(key), cr.goldens()[key]
    assert len(outs) == len(want)
    for i, o in enumerate(outs):
        st, g = fx.plane_stats(o), want[f"p{i}"]
        assert st["min"] == g["min"] and st["max"] == g["max"], (key, i, st, g)
        assert st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i, st, g)


# ---- the reference's behavioural tests -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gray8():
    return cr.golden_inputs("GRAY8", "full")[0]


def diff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


def test_defaults_are_mpeg_qscale8(gray8):
    assert np.array_equal(cr.frame([gray8])[0], cr.frame([gray8], codec=0, qscale=8)[0])
    assert cr.DEFAULTS == dict(codec=0, qscale=8, dc_prec=0, quality=50)


def test_mpeg_coarser_qscale_more_error(gray8):
    assert 0.0 < diff(cr.frame([gray8], codec=0, qscale=1)[0], gray8) < diff(cr.frame([gray8], codec=0, qscale=31)[0], gray8)


def test_jpeg_higher_quality_is_closer(gray8):
    assert diff(cr.frame([gray8], codec=1, quality=98)[0], gray8) < diff(cr.frame([gray8], codec=1, quality=8)[0], gray8)


def test_brightness_preserved(gray8):
    for kw in (dict(codec=0, qscale=31), dict(codec=1, quality=8)):
        assert fx.plane_stats(cr.frame([gray8], **kw)[0])["avg"] == pytest.approx(fx.plane_stats(gray8)["avg"], abs=6 / 255)


def test_chroma_false_leaves_chroma_untouched_and_true_modifies_it():
    src = cr.golden_inputs("YUV420P8", "full")
    off, on = cr.frame(src, chroma=False, codec=0, qscale=20), cr.frame(src, chroma=True, codec=0, qscale=20)
    assert diff(off[0], src[0]) > 0.0 and np.array_equal(off[1], src[1]) and np.array_equal(off[2], src[2])
    assert diff(on[1], src[1]) > 0.0 and diff(on[2], src[2]) > 0.0


def test_tiny_clips_replicate_the_edge():
    tiny = cr.golden_inputs("GRAY8", "tiny")[0]
    out = cr.frame([tiny], codec=0, qscale=8)[0]
    assert out.shape == tiny.shape == (7, 13)
    # a partial block is the block of the plane padded with its last column and row
    padded = np.pad(tiny, ((0, 1), (0, 3)), mode="edge")
    assert np.array_equal(cr.frame([padded], codec=0, qscale=8)[0][:7, :13], out)
    one = np.array([[77]], np.uint8)
    assert cr.frame([one], codec=1, quality=50)[0].shape == (1, 1)


def test_stride_independence(gray8):
    cropped = gray8[:, 27:]  # a view with the parent's pitch
    assert not cropped.flags["C_CONTIGUOUS"]
    for kw in (dict(codec=0, qscale=8), dict(codec=1, quality=25)):
        assert np.array_equal(cr.frame([cropped], **kw)[0], cr.frame([np.ascontiguousarray(cropped)], **kw)[0])


@pytest.mark.parametrize("kw", [dict(codec=0, qscale=1), dict(codec=0, qscale=31), dict(codec=0, dc_prec=0), dict(codec=0, dc_prec=3), dict(codec=1, quality=1),
                                dict(codec=1, quality=100)], ids=str)
def test_bounds_accepted(kw):
    from vszip_amd import capi

    assert cr.tables(**kw)["codec"] == capi.compress_tables(**kw).codec == kw["codec"]


# ---- the library's table generator -----------------------------------------------------------------------------------------------
def _same(got, want):
    g = got.as_dict()
    return g["codec"] == want["codec"] and np.array_equal(g["qmul"], want["qmul"]) and np.array_equal(g["deq"], want["deq"]) and g["dc_q"] == want["dc_q"] and \
        g["dc_scale"] == want["dc_scale"]


def test_library_tables_equal_the_spec_for_every_mpeg2_setting():
    from vszip_amd import capi

    for qscale in range(1, 32):
        for dc_prec in range(4):
            got, want = capi.compress_tables(0, qscale, dc_prec), cr.tables(0, qscale, dc_prec)
            assert _same(got, want), (qscale, dc_prec)
            assert np.array_equal(want["qmul"][0], want["qmul"][1]) and want["dc_q"] == 8 * want["dc_scale"] == 64 >> dc_prec
    t = cr.tables(0, 8, 0)
    assert t["deq"][0][0] == 128 and t["qmul"][0][0] == (2 << 21) // 128 and t["deq"][0][63] == 16 * 83


def test_library_tables_equal_the_spec_for_every_jpeg_quality():
    from vszip_amd import capi

    for quality in range(1, 101):
        assert _same(capi.compress_tables(1, quality=quality), cr.tables(1, quality=quality)), quality
    # the other codec's parameters are not looked at
    assert _same(capi.compress_tables(1, qscale=99, dc_prec=9, quality=50), cr.tables(1, quality=50))
    assert _same(capi.compress_tables(0, qscale=8, dc_prec=0, quality=0), cr.tables(0, 8, 0))
    t = cr.tables(1, quality=50)
    assert np.array_equal(t["deq"][0], cr.JPEG_LUMA) and np.array_equal(t["deq"][1], cr.JPEG_CHROMA)
    assert cr.tables(1, quality=100)["deq"].max() == 1 and cr.tables(1, quality=1)["deq"].max() == 255


ERRORS = [
    (dict(codec=2), r"codec must be 0 \(mpeg2\) or 1 \(jpeg\)"),
    (dict(codec=-1), r"codec must be 0 \(mpeg2\) or 1 \(jpeg\)"),
    (dict(codec=0, qscale=0), "qscale must be between 1 and 31"),
    (dict(codec=0, qscale=32), "qscale must be between 1 and 31"),
    (dict(codec=0, dc_prec=-1), "dc_prec must be between 0 and 3"),
    (dict(codec=0, dc_prec=4), "dc_prec must be between 0 and 3"),
    (dict(codec=1, quality=0), "quality must be between 1 and 100"),
    (dict(codec=1, quality=101), "quality must be between 1 and 100"),
]


@pytest.mark.parametrize("kw,msg", ERRORS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in ERRORS])
def test_argument_errors(kw, msg):
    from vszip_amd import capi

    with pytest.raises(ValueError, match="^Compress: " + msg + r"\.$"):
        cr.tables(**dict(cr.DEFAULTS, **kw))
    with pytest.raises(ValueError, match="^Compress: " + msg + r"\.$"):
        capi.compress_tables(**kw)


def test_errors_come_in_the_wrappers_order_and_through_the_c_abi():
    from vszip_amd import capi

    with pytest.raises(ValueError, match="qscale must be"):
        capi.compress_tables(0, qscale=0, dc_prec=9)
    lib = capi.load()
    tb, err = capi.CompressTables(), ctypes.create_string_buffer(64)
    assert lib.vszip_compress_tables(2, 8, 0, 50, ctypes.byref(tb), err, len(err)) == -1 and err.value == b"Compress: codec must be 0 (mpeg2) or 1 (jpeg)."
    assert lib.vszip_compress_tables(2, 8, 0, 50, ctypes.byref(tb), None, 0) == -1  # err may be NULL
    assert lib.vszip_compress_tables(0, 8, 0, 50, None, err, len(err)) == -1
    short = ctypes.create_string_buffer(12)
    assert lib.vszip_compress_tables(0, 99, 0, 50, ctypes.byref(tb), short, len(short)) == -1 and short.value == b"Compress: q"


def test_library_exports_the_entry_points():
    from vszip_amd import capi

    lib = ctypes.CDLL(str(capi.LIB_PATH))
    assert all(hasattr(lib, n) for n in ("vszip_compress", "vszip_compress_tables"))
    assert len(capi.SYMBOLS["vszip_compress"][1]) == 5 and len(capi.SYMBOLS["vszip_compress_tables"][1]) == 7 and capi.load().vszip_abi_version() == 4
    assert all(hasattr(capi.Device, n) for n in ("compress", "prepared_compress"))
    assert ctypes.sizeof(capi.CompressTables) == 4 + 2 * 2 * 64 * 4 + 8


# ---- branch coverage of the inputs of tests/test_gpu_compress.py -----------------------------------------------------------------
BRANCHES = ("killed", "kept", "positive", "negative", "dc_only_row", "general_row", "clamped_0", "clamped_255", "full_block", "partial_x", "partial_y")


@pytest.mark.parametrize("params", [cr.MPEG2_PARAMS, cr.JPEG_PARAMS], ids=["mpeg2", "jpeg"])
def test_gpu_inputs_take_every_branch(params):
    """Over the planes of gpu_planes() (every size of SIZES, noise and natural content alternating) and gpu_planes(1) (the other content at every
    size), each parameter set of the GPU tests alone takes every branch: a coefficient that quantises to zero and one kept, a positive and a negative level,
    a DC-only row of the inverse transform and a general one, a sample clamped at 0 and one at 255, full blocks and partial ones in both directions."""
    for kw in params:
        tb = cr.tables(**dict(cr.DEFAULTS, **kw))
        counts = {}
        for seed in (0, 1):
            for i, p in enumerate(cr.gpu_planes(seed)):
                cr.plane(p, tb, chroma=bool(i & 1), counts=counts)
        assert all(counts.get(b, 0) > 0 for b in BRANCHES), (kw, counts)


def test_noise_reaches_both_clamps_at_the_extreme_settings():
    """37 x 83 full-range noise (seed 0) alone: both clamps at qscale 1 and 31 and at quality 8 and 98 (counted: 2 + 2, 82 + 66, 154 + 156 and 6 + 1
    samples; not every seed reaches both at qscale 1, where a few samples of a plane clamp at all)"""
    p = cr.gpu_plane(0, 37, 83)
    assert p.shape == (83, 37)
    for kw in (dict(codec=0, qscale=1), dict(codec=0, qscale=31), dict(codec=1, quality=8), dict(codec=1, quality=98)):
        counts = {}
        cr.plane(p, cr.tables(**dict(cr.DEFAULTS, **kw)), counts=counts)
        assert counts["clamped_0"] > 0 and counts["clamped_255"] > 0, (kw, counts)
