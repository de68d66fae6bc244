"""The streaming filters (Limiter, LimitFilter, AdaptiveBinarize) with more planes than one launch's table holds
(192, csrc/plane_table.hpp): 230 planes of mixed sizes and per-plane constants in one call go out as two tables;
checked bit-exactly against the CPU oracle at both ends of each table (as tests/test_gpu_random.py does for BoxBlur)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 230
CHECKED = (0, 47, 48, 191, 192, 229)


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _shape(i):
    return (20 + i % 5, 61 + 9 * (i % 4))  # widths 61 / 70 / 79 / 88 on 32-byte aligned pitches: whole vectors and a scalar tail


def test_limiter(dev, oracle):
    rng = np.random.default_rng(9)
    planes = [rng.integers(0, 65536, size=_shape(i), dtype=np.uint16) for i in range(N)]
    lo = [1000 + 10 * i for i in range(N)]
    hi = [60000 - 10 * i for i in range(N)]
    ds = [dev.upload(p, 32) for p in planes]
    dd = [dev.empty(p.shape[0], p.shape[1], p.dtype, 32) for p in planes]
    dev.limiter(ds, dd, lo, hi)
    for i in CHECKED:
        assert np.array_equal(dev.download(dd[i]), oracle.limiter(planes[i], lo[i], hi[i])), i


@pytest.mark.parametrize("with_ref", [False, True])
def test_limit_filter(dev, oracle, with_ref):
    rng = np.random.default_rng(11)
    src = [rng.integers(0, 65536, size=_shape(i), dtype=np.uint16) for i in range(N)]
    flt = [rng.integers(0, 65536, size=p.shape, dtype=np.uint16) for p in src]
    ref = [rng.integers(0, 65536, size=p.shape, dtype=np.uint16) for p in src] if with_ref else None
    dark = [2000.0 + 50 * i for i in range(N)]
    bright = [30000.0 - 50 * i for i in range(N)]
    elast = [1.5 + 0.01 * i for i in range(N)]
    df, ds = [dev.upload(p, 32) for p in flt], [dev.upload(p, 32) for p in src]
    dr = [dev.upload(p, 32) for p in ref] if with_ref else None
    dd = [dev.empty(p.shape[0], p.shape[1], p.dtype, 32) for p in flt]
    dev.limit_filter(df, ds, dd, dark, bright, elast, dr)
    for i in CHECKED:
        want = oracle.limit_filter(flt[i], src[i], ref[i] if with_ref else None, dark[i], bright[i], elast[i])
        assert np.array_equal(dev.download(dd[i]), want), i


def test_adaptive_binarize(dev, oracle):
    rng = np.random.default_rng(10)
    a = [rng.integers(0, 256, size=_shape(i), dtype=np.uint8) for i in range(N)]
    b = [rng.integers(0, 256, size=p.shape, dtype=np.uint8) for p in a]
    da, db = [dev.upload(p, 32) for p in a], [dev.upload(p, 32) for p in b]
    dd = [dev.empty(p.shape[0], p.shape[1], np.uint8, 32) for p in a]
    dev.adaptive_binarize(da, db, dd, 7)
    for i in CHECKED:
        assert np.array_equal(dev.download(dd[i]), oracle.adaptive_binarize(a[i], b[i], 7)), i
