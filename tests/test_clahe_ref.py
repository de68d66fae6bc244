"""CPU: the CLAHE parity spec (tests/clahe_ref.py) reproduces every key of the reference's tests/goldens/clahe.json
(tests/golden/clahe_goldens.json) from tests/fixtures.py's inputs, and libvszip_hip.so exports vszip_clahe."""
import ctypes

import numpy as np
import pytest

import clahe_ref as cr
import fixtures as fx

KEYS = sorted(cr.goldens())


def test_all_42_keys_are_committed():
    assert len(KEYS) == 42
    assert {cr.parse_key(k)[0] for k in KEYS} == {"GRAY8", "GRAY16", "YUV420P8", "YUV444P8", "YUV420P16", "YUV444P16", "RGB24", "RGB48"}


@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_golden(key):
    fmt, geometry, limit, tiles = cr.parse_key(key)
    want = cr.goldens()[key]
    planes = cr.golden_inputs(fmt, geometry)
    assert len(planes) == len(want)
    for i, p in enumerate(planes):
        st = fx.plane_stats(cr.clahe(p, limit, tiles))
        g = want[f"p{i}"]
        assert st["min"] == g["min"] and st["max"] == g["max"], (key, i, st, g)
        assert st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i)


def test_tiles_argument_forms():
    assert cr.parse_tiles(3) == cr.parse_tiles([3]) == cr.parse_tiles([3, 3]) == (3, 3)
    assert cr.parse_tiles([8, 2]) == (8, 2)
    with pytest.raises(ValueError, match="tiles array can't have more than 2 values"):
        cr.parse_tiles([2, 2, 2])


def test_residual_closed_form_and_clip_limit():
    # clip_limit = max(1, limit * tw * th / hist_size) in u64, truncated (limit 0 -> 1)
    assert cr.clip_limit(1920, 1088, 0, (3, 3), 65536) == 1
    assert cr.clip_limit(1920, 1088, 7, (3, 3), 65536) == 7 * 640 * 362 // 65536
    assert cr.clip_limit(1920, 1088, 4_000_000_000, (3, 3), 65536) > cr.INT32_MAX
    # the reference's residual loop equals "bin i gets one iff i % step == 0 and i / step < residual"
    for hs in (256, 65536):
        for res in (1, 3, 100, 255, hs - 1):
            step = max(hs // res, 1)
            loop = np.zeros(hs, np.int64)
            i, r = 0, res
            while i < hs and r > 0:
                loop[i] += 1
                r -= 1
                i += step
            idx = np.arange(hs)
            assert np.array_equal(loop, ((idx % step == 0) & (idx // step < res)).astype(np.int64))


def test_library_exports_vszip_clahe():
    from vszip_amd import capi

    lib = ctypes.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "vszip_clahe")
    assert "vszip_clahe" in capi.SYMBOLS
    assert capi.load().vszip_abi_version() == 4
