"""GPU parity: vszip_clahe vs the CPU restatement (tests/clahe_ref.py), bit-exact; the reference's goldens (all 42 keys)
and its behavioural tests (reference tests/test_clahe.py)."""
import numpy as np
import pytest

import clahe_ref as cr
import fixtures as fx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _run(dev, planes, limit=7, tiles=3, align=32):
    ds = [dev.upload(np.ascontiguousarray(p), align) for p in planes]
    dd = [dev.empty(p.shape[0], p.shape[1], p.dtype, align) for p in planes]
    dev.clahe(ds, dd, limit, tiles)
    return [dev.download(d) for d in dd]


def _check(dev, planes, limit, tiles, align=32):
    t = cr.parse_tiles(tiles)
    for p, got in zip(planes, _run(dev, planes, limit, tiles, align)):
        want = cr.clahe(p, limit, t)
        assert np.array_equal(got, want), (p.shape, p.dtype, limit, t, align, int((got != want).sum()))


@pytest.mark.parametrize("key", sorted(cr.goldens()))
def test_reference_goldens(dev, key):
    fmt, geometry, limit, tiles = cr.parse_key(key)
    planes = cr.golden_inputs(fmt, geometry)
    out = _run(dev, planes, limit, list(tiles))
    for i, (p, got) in enumerate(zip(planes, out)):
        assert np.array_equal(got, cr.clahe(p, limit, tiles)), (key, i)
        st, g = fx.plane_stats(got), cr.goldens()[key][f"p{i}"]
        assert st["min"] == g["min"] and st["max"] == g["max"], (key, i)
        assert st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i)


SHAPES_SMALL = [(1, 1), (7, 13), (13, 7), (33, 70), (101, 257), (270, 481)]


# (more tiles than samples is an argument error: test_validation)
SMALL_CASES = [(s, t) for s in SHAPES_SMALL for t in [(1, 1), (3, 3), (8, 2), (2, 8), (16, 16)] if t[0] <= s[1] and t[1] <= s[0]]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape,tiles", SMALL_CASES)
def test_random_small(dev, dtype, shape, tiles):
    a = fx.splitmix64_plane(shape[0] * 1000 + shape[1] * 10 + tiles[0] + 100 * tiles[1], shape, dtype)
    _check(dev, [a], 7, list(tiles))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", [(7, 13), (13, 7)])
def test_one_sample_tiles(dev, dtype, shape):
    a = fx.splitmix64_plane(5, shape, dtype)
    _check(dev, [a], 7, [shape[1], shape[0]])
    _check(dev, [a], 7, [shape[1], 1])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("limit", [0, 1, 4, 7, 255, 2560])
def test_limits(dev, dtype, limit):
    a = fx.tiled_natural((203, 317), dtype)  # 317 % 3, 203 % 3 and 317 % 8 are not 0: remainder columns and rows
    _check(dev, [a], limit, [3, 3])
    _check(dev, [a], limit, [8, 5])


@pytest.mark.parametrize("dtype,hs", [(np.uint8, 256), (np.uint16, 65536)])
def test_largest_limit_below_int32_max(dev, dtype, hs):
    a = fx.splitmix64_plane(11, (400, 600), dtype)
    tw, th = 600 // 2, 400 // 1
    limit = (cr.INT32_MAX * hs) // (tw * th)
    while limit * tw * th // hs > cr.INT32_MAX:
        limit -= 1
    limit = min(limit, (1 << 32) - 1)
    assert limit < (1 << 32) - 1 and (limit + 1) * tw * th // hs > cr.INT32_MAX
    _check(dev, [a], limit, [2, 1])
    ds = [dev.upload(a)]
    with pytest.raises(Exception, match="limit too large"):
        dev.clahe(ds, ds, limit + 1, [2, 1])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("tiles", [(3, 3), (8, 8), (64, 36)])
def test_1080p(dev, dtype, tiles):
    _check(dev, [fx.splitmix64_plane(21, (1080, 1920), dtype)], 7, list(tiles))
    _check(dev, [fx.tiled_natural((1080, 1920), dtype)], 2560 if dtype == np.uint16 else 4, list(tiles))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_4k_luma_and_chroma(dev, dtype):
    planes = [fx.tiled_natural((2160, 3840), dtype, 0), fx.tiled_natural((1080, 1920), dtype, 1), fx.splitmix64_plane(3, (1080, 1920), dtype)]
    _check(dev, planes, 7, 3)
    _check(dev, planes, 7, [8, 8])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_content(dev, dtype):
    peak = np.iinfo(dtype).max
    flat = np.full((135, 241), 77, dtype)
    two = np.where(fx.splitmix64_plane(4, (135, 241), np.uint8) & 1, 3, peak - 3).astype(dtype)
    lo_end = np.zeros((64, 99), dtype)
    hi_end = np.full((64, 99), peak, dtype)
    ends = np.where(fx.splitmix64_plane(6, (64, 99), np.uint8) & 1, 0, peak).astype(dtype)
    _check(dev, [flat, two, lo_end, hi_end, ends], 7, 3)
    _check(dev, [flat, two, lo_end, hi_end, ends], 1, [4, 2])


def test_flat_large_gray16(dev):
    # reference test_clip_limit_large_frame_ok: 1920x1088 GRAY16 BlankClip(color=30000), limit 7, tiles [3]
    a = np.full((1088, 1920), 30000, np.uint16)
    (got,) = _run(dev, [a], 7, [3])
    assert np.array_equal(got, cr.clahe(a, 7, (3, 3)))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("align", [1, 8, 32])
def test_strides(dev, dtype, align):
    planes = [fx.splitmix64_plane(8, (97, 203), dtype), fx.tiled_natural((61, 150), dtype)]
    _check(dev, planes, 7, 3, align)
    _check(dev, planes, 4, [5, 2], align)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_stride_handling_crop(dev, dtype):
    """reference test_stride_handling: a plane cropped by 27 columns equals its repacked copy"""
    a = fx.tiled_natural((320, 640), dtype)
    full = dev.upload(a)
    cropped = dev.wrap(full.ptr + 27 * a.itemsize, a.shape[0], a.shape[1] - 27, full.stride, dtype)
    out = dev.empty(a.shape[0], a.shape[1] - 27, dtype)
    dev.clahe([cropped], [out], 15, 3)
    got = dev.download(out)
    (repacked,) = _run(dev, [np.ascontiguousarray(a[:, 27:])], 15, 3)
    assert np.array_equal(got, repacked)
    assert np.array_equal(got, cr.clahe(np.ascontiguousarray(a[:, 27:]), 15, (3, 3)))


def _frames(dtype, n):
    """Y, U, V of n frames of differing content and sizes"""
    out = []
    for f in range(n):
        h, w = 64 + 16 * (f % 5), 96 + 32 * (f % 3)
        y = fx.tiled_natural((h, w), dtype, f % 3) if f % 2 else fx.splitmix64_plane(f, (h, w), dtype)
        out += [y, fx.splitmix64_plane(100 + f, (h // 2, w // 2), dtype), fx.tiled_natural((h // 2, w // 2), dtype, 2)]
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_mixed_table_equals_plane_by_plane(dev, dtype):
    planes = _frames(dtype, 16)
    batched = _run(dev, planes, 7, [3, 2])
    for p, got in zip(planes, batched):
        assert np.array_equal(got, _run(dev, [p], 7, [3, 2])[0])
        assert np.array_equal(got, cr.clahe(p, 7, (3, 2)))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_more_planes_than_one_launch(dev, dtype):
    planes = [fx.splitmix64_plane(300 + i, (20 + i % 7, 30 + i % 11), dtype) for i in range(250)]
    for p, got in zip(planes, _run(dev, planes, 4, 3)):
        assert np.array_equal(got, cr.clahe(p, 4, (3, 3)))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_repeatable_and_in_place(dev, dtype):
    planes = _frames(dtype, 4)
    ds = [dev.upload(p) for p in planes]
    dd = [dev.empty(p.shape[0], p.shape[1], dtype) for p in planes]
    dev.clahe(ds, dd, 7, 3)
    first = [dev.download(d) for d in dd]
    dev.clahe(ds, dd, 7, 3)
    assert all(np.array_equal(a, dev.download(d)) for a, d in zip(first, dd))
    dev.clahe(ds, ds, 7, 3)  # dst == src
    for p, a, d in zip(planes, first, ds):
        assert np.array_equal(dev.download(d), a)
        assert np.array_equal(a, cr.clahe(p, 7, (3, 3)))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_lowered_scratch_cap(dev, dtype):
    planes = _frames(dtype, 8)
    want = _run(dev, planes, 7, [4, 4])
    assert dev.get_option("VSZIP_CLAHE_SCRATCH_MIB") == 1024
    with dev.options(VSZIP_CLAHE_SCRATCH_MIB=1):  # 16-bit: one plane per group (16 tiles = 6 MiB); 8-bit: 12 KiB a plane
        got = _run(dev, planes, 7, [4, 4])
    assert all(np.array_equal(a, b) for a, b in zip(want, got))


def test_tiles_forms_and_defaults(dev):
    a = cr.golden_inputs("GRAY16", "full")[0]
    ref = _run(dev, [a], 15, 3)[0]
    assert np.array_equal(_run(dev, [a], 15, [3])[0], ref)
    assert np.array_equal(_run(dev, [a], 15, [3, 3])[0], ref)
    d = dev.upload(a)
    o = dev.empty(a.shape[0], a.shape[1], a.dtype)
    dev.clahe([d], [o])  # defaults: limit 7, tiles 3
    assert np.array_equal(dev.download(o), _run(dev, [a], 7, [3, 3])[0])
    with pytest.raises(ValueError, match="tiles array can't have more than 2 values"):
        dev.clahe([d], [o], 7, [2, 2, 2])


def test_low_contrast_squeeze(dev):
    """reference test_equalization_increases_contrast: x / 4 + 16384, limit 2560, tiles 4"""
    a = (cr.golden_inputs("GRAY16", "full")[0] // 4 + 16384).astype(np.uint16)
    (got,) = _run(dev, [a], 2560, 4)
    assert np.array_equal(got, cr.clahe(a, 2560, (4, 4)))
    assert int(got.max()) > 60000 and int(got.min()) < 4000


def test_validation(dev):
    from vszip_amd import capi

    y = dev.upload(np.full((1088, 1920), 30000, np.uint16))
    u = dev.upload(np.full((544, 960), 30000, np.uint16))
    table = dev.plane_table([y, u], [y, u])

    def call(dtype, limit, tx, ty, tab=table, n=2):
        rc = dev.lib.vszip_clahe(dev.ctx, dtype, tab, n, limit, tx, ty)
        return rc, dev.lib.vszip_last_error(dev.ctx).decode()

    for dt in (capi.F16, capi.F32, 4):
        rc, msg = call(dt, 7, 3, 3)
        assert rc == capi.ERR_ARG and "only 8 or 16 bit int formats supported" in msg
    for tx, ty in ((0, 3), (3, 0), (-1, 1)):
        rc, msg = call(capi.U16, 7, tx, ty)
        assert rc == capi.ERR_ARG and "tiles values must be >= 1" in msg
    for tx, ty in ((961, 3), (3, 545), (1921, 1)):  # above the chroma plane only, then above the luma plane too
        rc, msg = call(capi.U16, 7, tx, ty)
        assert rc == capi.ERR_ARG and "tiles must not exceed the (chroma) plane width/height" in msg
    rc, msg = call(capi.U16, 4_000_000_000, 3, 3, dev.plane_table([y], [y]), 1)  # reference test_clip_limit_too_big_errors
    assert rc == capi.ERR_ARG and "limit too large" in msg
    s = dev.upload(np.full((14, 26), 3, np.uint16))
    c = dev.upload(np.full((7, 13), 3, np.uint16))
    assert call(capi.U16, 7, 13, 7, dev.plane_table([s, c], [s, c]))[0] == capi.OK  # the largest tile counts the chroma plane allows
    assert call(capi.U16, 7, 14, 7, dev.plane_table([s, c], [s, c]))[0] == capi.ERR_ARG
    dev.sync()
