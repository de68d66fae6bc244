"""GPU parity: vszip_comb_mask / vszip_comb_mask_mt vs the CPU restatement (tests/combmask_ref.py), bit-exact: the reference's
goldens (all 39 keys), its eight (metric, expand, motion) variants and both CombMaskMT forms on small shapes, threshold
extremes, full-size frames, edge-row motion, pointer and pitch layouts, tables and the create-time errors."""
import ctypes as C

import numpy as np
import pytest

import combmask_ref as cr
import fixtures as fx

pytestmark = pytest.mark.gpu

# (metric, expand, mthresh): the reference's eight getFrame variants
VARIANTS = [(metric, expand, mthresh) for metric in (0, 1) for expand in (False, True) for mthresh in (0, 9)]
MT_FORMS = [(30, 30), (10, 90)]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _up(dev, planes, align=32):
    return [dev.upload(np.ascontiguousarray(p), align) for p in planes]


def _run(dev, srcs, prvs=None, align=32, **kw):
    ds = _up(dev, srcs, align)
    dp = _up(dev, prvs, align) if prvs is not None else None
    dd = [dev.empty(p.shape[0], p.shape[1], np.uint8, align) for p in srcs]
    dev.comb_mask(ds, dd, dp, **kw)
    return [dev.download(d) for d in dd]


def _run_mt(dev, srcs, thy1=30, thy2=30, align=32):
    ds = _up(dev, srcs, align)
    dd = [dev.empty(p.shape[0], p.shape[1], np.uint8, align) for p in srcs]
    dev.comb_mask_mt(ds, dd, thy1, thy2)
    return [dev.download(d) for d in dd]


def _check(dev, srcs, prvs, align=32, **kw):
    got = _run(dev, srcs, prvs, align, **kw)
    for i, (s, g) in enumerate(zip(srcs, got)):
        want = cr.comb_mask(s, prvs[i] if prvs is not None else None, **kw)
        assert np.array_equal(g, want), (i, s.shape, kw, align, int((g != want).sum()), np.argwhere(g != want)[:4].tolist())


def _check_mt(dev, srcs, thy1, thy2, align=32):
    got = _run_mt(dev, srcs, thy1, thy2, align)
    for i, (s, g) in enumerate(zip(srcs, got)):
        want = cr.comb_mask_mt(s, thy1, thy2)
        assert np.array_equal(g, want), (i, s.shape, thy1, thy2, align, int((g != want).sum()), np.argwhere(g != want)[:4].tolist())


def _combed(seed, shape, natural=False):
    """(frame n, frame n - 1): content with combing (alternate rows pushed apart) and motion in part of the picture"""
    h, w = shape
    base = fx.tiled_natural(shape, np.uint8, seed % 3) if natural else (fx.splitmix64_plane(seed, shape, np.uint8) >> 2) + 64
    s = base.astype(np.int32)
    bump = (fx.splitmix64_plane(seed + 1000, shape, np.uint8).astype(np.int32) % 60)
    s[1::2] += bump[1::2]
    s = np.clip(s, 0, 255).astype(np.uint8)
    p = s.copy()
    mov = fx.splitmix64_plane(seed + 2000, shape, np.uint8) > 170
    p[mov] = np.clip(p[mov].astype(np.int32) + 40, 0, 255).astype(np.uint8)
    return s, p


# ---- goldens --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(cr.goldens()))
def test_reference_goldens(dev, key):
    fmt, geometry, filt, kw = cr.parse_key(key)
    srcs, prvs = cr.golden_inputs(fmt, geometry, filt)
    got = _run(dev, srcs, prvs, **kw) if filt == "CombMask" else _run_mt(dev, srcs, **kw)
    want = cr.run_key(key)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (key, i)
        st, gold = fx.plane_stats(g), cr.goldens()[key][f"p{i}"]
        assert st["min"] == gold["min"] and st["max"] == gold["max"], (key, i)
        assert st["avg"] == pytest.approx(gold["avg"], rel=1e-9, abs=0), (key, i)


# ---- small shapes and thresholds ------------------------------------------------------------------------------------
SMALL = [(h, w) for h in (3, 4, 5, 7) for w in (1, 2, 3, 15, 16, 17, 33, 257)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_shapes_every_variant(dev, shape):
    noise = _combed(shape[0] * 1000 + shape[1], shape)
    flat = fx.splitmix64_plane(7 + shape[1], shape, np.uint8)  # full-range noise: every branch of the metric
    prev = fx.splitmix64_plane(8 + shape[0], shape, np.uint8)
    for metric, expand, mthresh in VARIANTS:
        kw = dict(cthresh=6, mthresh=mthresh, expand=expand, metric=metric)
        _check(dev, [noise[0], flat], [noise[1], prev], **kw)
    for thy1, thy2 in MT_FORMS:
        _check_mt(dev, [noise[0], flat], thy1, thy2)


@pytest.mark.parametrize("metric,cthresh", [(0, 0), (0, 255), (1, 0), (1, 255), (1, 65025), (1, 65024)])
@pytest.mark.parametrize("mthresh", [0, 1, 255, 254])
def test_threshold_extremes(dev, metric, cthresh, mthresh):
    shape = (37, 203)
    s = fx.splitmix64_plane(1, shape, np.uint8)
    s[5:9, 10:40] = np.array([0, 255, 0, 255], np.uint8)[:, None]  # the largest comb: (255)(255) = 65025, |d| = 255
    p = fx.splitmix64_plane(2, shape, np.uint8)
    p[20:24, :50] = 255 - (s[20:24, :50] // 128) * 255  # differences of at least 128, some of exactly 255
    s[22, :25] = 0
    p[22, :25] = 255
    for expand in (False, True):
        _check(dev, [s], [p], cthresh=cthresh, mthresh=mthresh, expand=expand, metric=metric)


@pytest.mark.parametrize("thy1,thy2", [(0, 0), (255, 255), (0, 255), (200, 255), (29, 30), (0, 1), (254, 255), (17, 130)])
def test_mt_threshold_extremes(dev, thy1, thy2):
    s = fx.splitmix64_plane(3, (41, 203), np.uint8)
    s[5:9, 10:40] = np.array([0, 255, 0, 255], np.uint8)[:, None]
    ramp = (np.arange(64)[None, :] * 4).astype(np.uint8)  # products that sweep through [thY1, thY2]
    t = np.zeros((9, 64), np.uint8)
    t[1::2] = ramp // 16
    _check_mt(dev, [s, t, fx.tiled_natural((50, 77), np.uint8)], thy1, thy2)


# ---- sizes and content ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["1080p", "4k"])
def test_full_size_luma_and_chroma(dev, size):
    h, w = (1080, 1920) if size == "1080p" else (2160, 3840)
    pairs = [_combed(1, (h, w), natural=True), _combed(2, (h // 2, w // 2), natural=True), _combed(3, (h // 2, w // 2))]
    srcs, prvs = [a for a, _ in pairs], [b for _, b in pairs]
    for metric, expand, mthresh in VARIANTS:
        _check(dev, srcs, prvs, cthresh=6, mthresh=mthresh, expand=expand, metric=metric)
    for thy1, thy2 in MT_FORMS:
        _check_mt(dev, srcs, thy1, thy2)


def test_content(dev):
    shape = (135, 241)
    nat = fx.tiled_natural(shape, np.uint8)
    nat_prev = np.roll(nat, 1, axis=0)  # the reference's temporal fixture: shifted by a row
    noise, noise_prev = fx.splitmix64_plane(4, shape, np.uint8), fx.splitmix64_plane(5, shape, np.uint8)
    flat, flat_prev = np.full(shape, 77, np.uint8), np.full(shape, 90, np.uint8)
    srcs, prvs = [nat, noise, flat, flat], [nat_prev, noise_prev, flat_prev, flat]
    for metric, expand, mthresh in VARIANTS:
        _check(dev, srcs, prvs, cthresh=6, mthresh=mthresh, expand=expand, metric=metric)
        _check(dev, srcs, prvs, cthresh=20, mthresh=50 if mthresh else 0, expand=expand, metric=metric)
    for thy1, thy2 in MT_FORMS:
        _check_mt(dev, srcs, thy1, thy2)


@pytest.mark.parametrize("shape", [(3, 40), (8, 9), (16, 33), (17, 64), (33, 130), (50, 1000)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("row", ["first", "last", "second", "band_seam"])
def test_motion_in_one_row_only(dev, shape, row):
    """the lopsided dilation: nothing above row 0, row h - 1 itself below it; and a row on either side of a band of rows"""
    h, w = shape
    s = np.zeros(shape, np.uint8)
    s[::2] = 200  # combed everywhere, both metrics
    y = {"first": 0, "last": h - 1, "second": 1, "band_seam": min(h - 1, 16)}[row]
    p = s.copy()
    p[y] ^= 0x80
    for metric in (0, 1):
        for expand in (False, True):
            got = _run(dev, [s], [p], cthresh=6, mthresh=9, expand=expand, metric=metric)[0]
            assert np.array_equal(got, cr.comb_mask(s, p, 6, 9, expand, metric))
            assert sorted(set(np.nonzero(got)[0])) == [r for r in (y - 1, y, y + 1) if 0 <= r < h]
    y2 = max(0, y - 1)  # the row before a seam as well
    p2 = s.copy()
    p2[y2, w // 2:] ^= 0x80
    _check(dev, [s], [p2], cthresh=6, mthresh=9, expand=True, metric=0)


# ---- pointers and memory layout -------------------------------------------------------------------------------------
def test_prev_is_the_same_pointer(dev):
    s, _ = _combed(9, (70, 333), natural=True)
    (d,) = _up(dev, [s])
    o = dev.empty(70, 333, np.uint8)
    for metric in (0, 1):
        dev.lib.vszip_dev_memset(dev.ctx, C.c_void_p(o.ptr), 0x55, o.stride * o.h)
        dev.comb_mask([d], [o], [d], cthresh=2, mthresh=1, metric=metric)
        assert not dev.download(o).any()
        dev.comb_mask([d], [o], [d], cthresh=2, mthresh=0, metric=metric)
        got = dev.download(o)
        assert got.any() and np.array_equal(got, cr.comb_mask(s, None, 2, 0, True, metric))


@pytest.mark.parametrize("align", [1, 8, 32])
def test_strides(dev, align):
    pairs = [_combed(11, (97, 203)), _combed(12, (61, 150), natural=True), _combed(13, (40, 1031))]
    srcs, prvs = [a for a, _ in pairs], [b for _, b in pairs]
    for metric, expand, mthresh in VARIANTS:
        _check(dev, srcs, prvs, align, cthresh=6, mthresh=mthresh, expand=expand, metric=metric)
    for thy1, thy2 in MT_FORMS:
        _check_mt(dev, srcs, thy1, thy2, align)


@pytest.mark.parametrize("shift", [1, 8, 32])
def test_base_alignments(dev, shift):
    """planes that start `shift` bytes into their allocation (pitch a multiple of 32)"""
    s, p = _combed(21, (66, 300), natural=True)
    big_s, big_p = _up(dev, [np.pad(s, ((0, 0), (shift, 0))), np.pad(p, ((0, 0), (shift, 0)))])
    big_o = dev.empty(66, 300 + shift, np.uint8)
    view = lambda b: dev.wrap(b.ptr + shift, 66, 300, b.stride, np.uint8)
    for metric, expand, mthresh in VARIANTS:
        dev.comb_mask([view(big_s)], [view(big_o)], [view(big_p)], cthresh=6, mthresh=mthresh, expand=expand, metric=metric)
        assert np.array_equal(dev.download(big_o)[:, shift:], cr.comb_mask(s, p, 6, mthresh, expand, metric)), (metric, expand, mthresh)
    for thy1, thy2 in MT_FORMS:
        dev.comb_mask_mt([view(big_s)], [view(big_o)], thy1, thy2)
        assert np.array_equal(dev.download(big_o)[:, shift:], cr.comb_mask_mt(s, thy1, thy2))


@pytest.mark.parametrize("x0", [27, 32])
def test_cropped_window(dev, x0):
    """a window into a larger plane equals its repacked copy, and the plane around the output window is left alone"""
    a, b = _combed(31, (320, 640), natural=True)
    fa, fb = _up(dev, [a, b])
    h, w, y0 = 200, 640 - x0 - 5, 60
    win = lambda f: dev.wrap(f.ptr + y0 * f.stride + x0, h, w, f.stride, np.uint8)
    sa, sb = np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(b[y0:y0 + h, x0:x0 + w])
    for metric, expand, mthresh in VARIANTS:
        marker = fx.splitmix64_plane(77, (320, 640), np.uint8)
        (out,) = _up(dev, [marker])
        dev.comb_mask([win(fa)], [win(out)], [win(fb)], cthresh=6, mthresh=mthresh, expand=expand, metric=metric)
        got = dev.download(out)
        want = marker.copy()
        want[y0:y0 + h, x0:x0 + w] = cr.comb_mask(sa, sb, 6, mthresh, expand, metric)
        assert np.array_equal(got, want), (metric, expand, mthresh)
    (out,) = _up(dev, [marker])
    dev.comb_mask_mt([win(fa)], [win(out)], 10, 90)
    want = marker.copy()
    want[y0:y0 + h, x0:x0 + w] = cr.comb_mask_mt(sa, 10, 90)
    assert np.array_equal(dev.download(out), want)


def test_ref_is_ignored_without_motion(dev):
    s, _ = _combed(41, (90, 401), natural=True)
    (d,) = _up(dev, [s])
    garbage = dev.upload(fx.splitmix64_plane(42, (7, 13), np.uint8))  # far too small to be read as a 90 x 401 plane
    o1, o2 = dev.empty(90, 401, np.uint8), dev.empty(90, 401, np.uint8)
    for metric in (0, 1):
        for expand in (False, True):
            dev.comb_mask([d], [o1], None, cthresh=6, mthresh=0, expand=expand, metric=metric)
            table = dev.plane_table([d], [o2])
            table[0].ref, table[0].ref_stride = garbage.ptr + 3, 5
            dev.check(dev.lib.vszip_comb_mask(dev.ctx, table, 1, 6, 0, int(expand), metric))
            a, b = dev.download(o1), dev.download(o2)
            assert np.array_equal(a, b) and np.array_equal(a, cr.comb_mask(s, None, 6, 0, expand, metric))


# ---- tables and repeatability ---------------------------------------------------------------------------------------
def _frames(n):
    """Y, U, V (and their previous frame) of n frames of differing content and sizes"""
    srcs, prvs = [], []
    for f in range(n):
        h, w = 48 + 16 * (f % 5), 96 + 31 * (f % 3)
        for k, shape in enumerate([(h, w), (h // 2, w // 2), (h // 2, w // 2)]):
            s, p = _combed(10 * f + k, shape, natural=(f + k) % 2 == 0)
            srcs.append(s)
            prvs.append(p)
    return srcs, prvs


def test_mixed_table_equals_plane_by_plane(dev):
    srcs, prvs = _frames(16)
    for kw in (dict(), dict(cthresh=8, mthresh=0, metric=1), dict(cthresh=8, mthresh=30, expand=False)):
        batched = _run(dev, srcs, prvs, **kw)
        for s, p, got in zip(srcs, prvs, batched):
            assert np.array_equal(got, _run(dev, [s], [p], **kw)[0])
            assert np.array_equal(got, cr.comb_mask(s, p, **kw))
    for thy1, thy2 in MT_FORMS:
        batched = _run_mt(dev, srcs, thy1, thy2)
        for s, got in zip(srcs, batched):
            assert np.array_equal(got, _run_mt(dev, [s], thy1, thy2)[0])
            assert np.array_equal(got, cr.comb_mask_mt(s, thy1, thy2))


@pytest.mark.parametrize("n,launches", [(250, 2), (192, 1), (1, 1), (193, 2)])
def test_one_launch_per_table(dev, n, launches):
    pairs = [_combed(300 + i, (20 + i % 7, 30 + i % 11)) for i in range(n)]
    srcs, prvs = [a for a, _ in pairs], [b for _, b in pairs]
    ds, dp = _up(dev, srcs), _up(dev, prvs)
    dd = [dev.empty(p.shape[0], p.shape[1], np.uint8) for p in srcs]
    dev.probe_enable(True)
    try:
        dev.comb_mask(ds, dd, dp)
        assert dev.probe_read()[1] == launches
        for s, p, d in zip(srcs, prvs, dd):
            assert np.array_equal(dev.download(d), cr.comb_mask(s, p))
        dev.comb_mask(ds, dd, None, cthresh=8, mthresh=0, expand=False, metric=1)
        assert dev.probe_read()[1] == launches
        dev.comb_mask_mt(ds, dd, 10, 90)
        assert dev.probe_read()[1] == launches
        for s, d in zip(srcs, dd):
            assert np.array_equal(dev.download(d), cr.comb_mask_mt(s, 10, 90))
    finally:
        dev.probe_enable(False)


def test_repeatable(dev):
    srcs, prvs = _frames(4)
    ds, dp = _up(dev, srcs), _up(dev, prvs)
    dd = [dev.empty(p.shape[0], p.shape[1], np.uint8) for p in srcs]
    run = dev.prepared_comb_mask(ds, dd, dp)
    run()
    first = [dev.download(d) for d in dd]
    for _ in range(3):
        run()
    assert all(np.array_equal(a, dev.download(d)) for a, d in zip(first, dd))
    assert all(np.array_equal(a, cr.comb_mask(s, p)) for a, s, p in zip(first, srcs, prvs))
    dev.comb_mask_mt(ds, dd, 0, 255)
    first = [dev.download(d) for d in dd]
    dev.comb_mask_mt(ds, dd, 0, 255)
    assert all(np.array_equal(a, dev.download(d)) for a, d in zip(first, dd))


def test_defaults(dev):
    s, p = _combed(51, (64, 200), natural=True)
    ds, dp = _up(dev, [s]), _up(dev, [p])
    o = dev.empty(64, 200, np.uint8)
    dev.comb_mask(ds, [o], dp)
    assert np.array_equal(dev.download(o), cr.comb_mask(s, p, 6, 9, True, 0))
    dev.comb_mask_mt(ds, [o])
    assert np.array_equal(dev.download(o), cr.comb_mask_mt(s, 30, 30))


# ---- validation -----------------------------------------------------------------------------------------------------
def test_validation(dev):
    from vszip_amd import capi

    y = dev.upload(np.full((8, 64), 100, np.uint8))
    u = dev.upload(np.full((4, 32), 100, np.uint8))
    short = dev.upload(np.full((2, 32), 100, np.uint8))  # the chroma of a 4-row YUV420 clip
    table = dev.plane_table([y, u], [y, u], [y, u])  # (never launched: every call below is refused)
    o = dev.empty(8, 64, np.uint8)

    def cm(tab, n, *args):
        rc = dev.lib.vszip_comb_mask(dev.ctx, tab, n, *args)
        return rc, dev.lib.vszip_last_error(dev.ctx).decode()

    def mt(tab, n, *args):
        rc = dev.lib.vszip_comb_mask_mt(dev.ctx, tab, n, *args)
        return rc, dev.lib.vszip_last_error(dev.ctx).decode()

    for cth, metric, text in ((256, 0, "CombMask: cthresh must be between 0 and 255 when metric = false."), (-1, 0, "CombMask: cthresh must be between 0 and 255 when metric = false."),
                              (65026, 1, "CombMask: cthresh must be between 0 and 65025 when metric = true."), (-1, 1, "CombMask: cthresh must be between 0 and 65025 when metric = true.")):
        rc, msg = cm(table, 2, cth, 9, 1, metric)
        assert rc == capi.ERR_ARG and msg == text
    for mth in (256, -1):
        rc, msg = cm(table, 2, 6, mth, 1, 0)
        assert rc == capi.ERR_ARG and msg == "CombMask: mthresh must be between 0 and 255."
    for a, b, text in ((-1, 30, "CombMaskMT: thY1 value should be in range [0;255]"), (256, 256, "CombMaskMT: thY1 value should be in range [0;255]"),
                       (30, -1, "CombMaskMT: thY2 value should be in range [0;255]"), (30, 256, "CombMaskMT: thY2 value should be in range [0;255]"),
                       (31, 30, "CombMaskMT: thY1 can't be greater than thY2"), (255, 0, "CombMaskMT: thY1 can't be greater than thY2")):
        rc, msg = mt(table, 2, a, b)
        assert rc == capi.ERR_ARG and msg == text
    small = dev.plane_table([y, short], [y, short], [y, short])
    for metric, mth in ((0, 9), (1, 9), (0, 0)):
        rc, msg = cm(small, 2, 6, mth, 1, metric)
        assert rc == capi.ERR_ARG and msg == "CombMask: clip too small; every plane must be at least 3 rows tall."
    rc, msg = mt(small, 2, 30, 30)
    assert rc == capi.ERR_ARG and msg == "CombMaskMT: clip too small; every plane must be at least 3 rows tall."
    for field in ("src", "dst"):
        bad = dev.plane_table([y], [o], [y])
        setattr(bad[0], field, None)
        rc, msg = cm(bad, 1, 6, 9, 1, 0)
        assert rc == capi.ERR_ARG and "src and dst must not be NULL" in msg
        rc, msg = mt(bad, 1, 30, 30)
        assert rc == capi.ERR_ARG and "src and dst must not be NULL" in msg
    noref = dev.plane_table([y], [o])
    rc, msg = cm(noref, 1, 6, 9, 1, 0)
    assert rc == capi.ERR_ARG and "ref (the previous frame's plane) must not be NULL when mthresh > 0" in msg
    assert cm(noref, 1, 6, 0, 1, 0)[0] == capi.OK  # ... and is not needed without motion
    three = dev.upload(np.full((3, 64), 100, np.uint8))  # exactly 3 rows is accepted
    o3 = dev.empty(3, 64, np.uint8)
    assert cm(dev.plane_table([three], [o3], [three]), 1, 6, 9, 1, 0)[0] == capi.OK
    assert mt(dev.plane_table([three], [o3]), 1, 30, 30)[0] == capi.OK
    assert cm(dev.plane_table([y], [o], [y]), 1, 255, 255, 0, 0)[0] == capi.OK and cm(dev.plane_table([y], [o], [y]), 1, 65025, 255, 0, 1)[0] == capi.OK
    assert mt(dev.plane_table([y], [o]), 1, 0, 255)[0] == capi.OK
    dev.sync()
