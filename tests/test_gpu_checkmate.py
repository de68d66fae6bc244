"""GPU parity: vszip_checkmate vs the CPU restatement (tests/checkmate_ref.py), bit-exact: the reference's goldens (all 25
keys), both instantiations (tthr2 == 0: three input streams; tthr2 > 0: five) on small shapes, the band and strip seams
with the right clamp in every position, parameter extremes, unaligned layouts, aliased neighbours, the clip form, a table
longer than one launch, full-size frames, the prepared form and the create-time errors."""
import numpy as np
import pytest

import checkmate_ref as ck
import fixtures as fx

pytestmark = pytest.mark.gpu

R = 32        # kBandRows of csrc/checkmate.hip: the rows of a band (a wave walks the 16 of one parity)
S = 62 * 8    # kStripGroups * kGroup: the samples of a row a wave stores


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def full_noise(seed, shape, n=5):
    return [fx.splitmix64_plane(seed + k, shape, np.uint8) for k in range(n)]


def binary_noise(seed, shape, n=5):
    """independent 0 / 255 samples: with thr = tmax = 255 curr reaches -1020 and the output saturates at both ends
    (tests/test_checkmate_ref.py::test_binary_noise_reaches_every_extreme)"""
    return [np.where(fx.splitmix64_plane(seed + k, shape, np.uint8) & 1, 255, 0).astype(np.uint8) for k in range(n)]


def correlated(seed, shape, n=5):
    """frames -6 .. 6 around a full-range base: tthr2 = 8 takes the blend on some samples and not on others"""
    base = fx.splitmix64_plane(seed, shape, np.uint8).astype(np.int32)
    return [np.clip(base + fx.splitmix64_plane(seed + 100 + k, shape, np.uint8).astype(np.int32) % 13 - 6, 0, 255).astype(np.uint8) for k in range(n)]


CONTENT = {"noise": full_noise, "binary": binary_noise, "correlated": correlated}


def _up(dev, planes, align=32):
    return [dev.upload(np.ascontiguousarray(p), align) for p in planes]


def _run(dev, sets, align=32, **kw):
    """sets: [(p2, p1, cur, n1, n2)] -> the outputs"""
    cols = [_up(dev, [s[k] for s in sets], align) for k in range(5)]
    dd = [dev.empty(s[2].shape[0], s[2].shape[1], np.uint8, align) for s in sets]
    dev.checkmate(cols[2], dd, cols[1], cols[3], cols[0], cols[4], **kw)
    return [dev.download(d) for d in dd]


def _check(dev, sets, align=32, **kw):
    got = _run(dev, sets, align, **kw)
    for i, (s, g) in enumerate(zip(sets, got)):
        want = ck.checkmate(*s, **kw)
        assert np.array_equal(g, want), (i, s[2].shape, kw, align, int((g != want).sum()), np.argwhere(g != want)[:4].tolist())


# ---- goldens --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(ck.goldens()))
def test_reference_goldens(dev, key):
    fmt, geometry, kw = ck.parse_key(key)
    f0, f1, f2 = ck.golden_inputs(fmt, geometry)
    got = _run(dev, [(a, a, b, c, c) for a, b, c in zip(f0, f1, f2)], **kw)  # frame 1 of 3: p2 = p1 = frame 0, n1 = n2 = frame 2
    for i, (g, w) in enumerate(zip(got, ck.run_key(key))):
        assert np.array_equal(g, w), (key, i)
        st, gold = fx.plane_stats(g), ck.goldens()[key][f"p{i}"]
        assert st["min"] == gold["min"] and st["max"] == gold["max"], (key, i)
        assert st["avg"] == pytest.approx(gold["avg"], rel=1e-9, abs=0), (key, i)


# ---- small shapes, seams, parameters --------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [5, 6, 7, 9])
@pytest.mark.parametrize("tthr2", [0, 1, 8, 256, 100000])
def test_small_shapes(dev, h, tthr2):
    sets = []
    for w in (3, 4, 5, 15, 16, 17, 18, 19, 33, 257):
        for k, make in enumerate(CONTENT.values()):
            sets.append(tuple(make(100 * h + w + k, (h, w))))
    _check(dev, sets, thr=12, tmax=12, tthr2=tthr2)
    _check(dev, sets, thr=255, tmax=255, tthr2=tthr2)


@pytest.mark.parametrize("h", [R + 3, R + 4, R + 5, 2 * R + 4])
@pytest.mark.parametrize("tthr2", [0, 8])
def test_band_and_strip_seams(dev, h, tthr2):
    """a band seam at every distance from the copied rows; the right clamp in the last lane group of a strip, in the first of
    the next (whose neighbour lane lies in the other wave's strip), and one and seventeen samples on (two lane groups)"""
    sets = [tuple(correlated(h + w, (h, w))) for w in (S - 1, S, S + 1, S + 17)]
    sets.append(tuple(binary_noise(h, (h, S + 1))))
    _check(dev, sets, thr=12, tmax=12, tthr2=tthr2)


@pytest.mark.parametrize("thr,tmax", [(0, 1), (255, 255), (0, 255), (255, 1), (12, 3), (12, 7)])
def test_parameter_extremes(dev, thr, tmax):
    shape = (37, 203)
    sets = [tuple(make(9, shape)) for make in CONTENT.values()]
    for tthr2 in (0, 8):
        _check(dev, sets, thr=thr, tmax=tmax, tthr2=tthr2)


# ---- pointers and memory layout -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("tthr2", [0, 8])
def test_base_offsets_and_odd_pitches(dev, shift, tthr2):
    """every plane `shift` bytes into its allocation, with an odd pitch"""
    h, w = 45, 203
    f = correlated(31 + shift, (h, w))
    bigs = _up(dev, [np.pad(a, ((0, 0), (shift, 1))) for a in f], 1)
    assert bigs[0].stride == w + shift + 1 and bigs[0].stride % 2 == 1
    out = dev.empty(h, w + shift + 1, np.uint8, 1)
    view = lambda b: dev.wrap(b.ptr + shift, h, w, b.stride, np.uint8)
    v = [view(b) for b in bigs]
    dev.checkmate([v[2]], [view(out)], [v[1]], [v[3]], [v[0]], [v[4]], tthr2=tthr2)
    assert np.array_equal(dev.download(out)[:, shift:shift + w], ck.checkmate(*f, tthr2=tthr2))


@pytest.mark.parametrize("align", [1, 8])
def test_strides(dev, align):
    sets = [tuple(correlated(11, (97, 203))), tuple(full_noise(12, (61, 150))), tuple(binary_noise(13, (40, 1031)))]
    for tthr2 in (0, 8):
        _check(dev, sets, align, thr=12, tmax=12, tthr2=tthr2)


@pytest.mark.parametrize("which", [1, 3, 0])
@pytest.mark.parametrize("tthr2", [0, 8])
def test_one_neighbour_unaligned(dev, which, tthr2):
    """src, dst and the other neighbours aligned: the entry must take the byte path as a whole (which = 0: p2, read only with tthr2 > 0)"""
    h, w = 40, 300
    f = correlated(50 + which, (h, w))
    d = _up(dev, f)
    big = dev.upload(np.pad(f[which], ((0, 0), (1, 0))))
    d[which] = dev.wrap(big.ptr + 1, h, w, big.stride, np.uint8)
    o = dev.empty(h, w, np.uint8)
    dev.checkmate([d[2]], [o], [d[1]], [d[3]], [d[0]], [d[4]], tthr2=tthr2)
    assert np.array_equal(dev.download(o), ck.checkmate(*f, tthr2=tthr2))


@pytest.mark.parametrize("tthr2", [0, 8])
def test_neighbours_may_be_the_source(dev, tthr2):
    h, w = 70, 333
    f = correlated(61, (h, w))
    d = _up(dev, f)
    o = dev.empty(h, w, np.uint8)
    for name, idx in (("p1", (0, 2, 2, 3, 4)), ("n1", (0, 1, 2, 2, 4)), ("all", (2, 2, 2, 2, 2)), ("p1 is p2", (1, 1, 2, 3, 3))):
        g = [d[i] for i in idx]
        dev.checkmate([g[2]], [o], [g[1]], [g[3]], [g[0]], [g[4]], tthr2=tthr2)
        assert np.array_equal(dev.download(o), ck.checkmate(*[f[i] for i in idx], tthr2=tthr2)), name


def test_p2_and_n2_are_not_read_without_tthr2(dev):
    h, w = 90, 401
    f = full_noise(71, (h, w))
    d = _up(dev, f)
    garbage = dev.upload(fx.splitmix64_plane(42, (7, 13), np.uint8))  # far too small to be read as a 90 x 401 plane
    o1, o2 = dev.empty(h, w, np.uint8), dev.empty(h, w, np.uint8)
    dev.checkmate([d[2]], [o1], [d[1]], [d[3]])
    nbrs = dev.temporal_nbrs([d[1]], [d[3]])
    nbrs[0].p2, nbrs[0].p2_stride, nbrs[0].n2, nbrs[0].n2_stride = garbage.ptr + 3, 5, garbage.ptr + 1, 7
    dev.check(dev.lib.vszip_checkmate(dev.ctx, dev.plane_table([d[2]], [o2]), nbrs, 1, 12, 12, 0))
    a, b = dev.download(o1), dev.download(o2)
    assert np.array_equal(a, b) and np.array_equal(a, ck.checkmate(None, f[1], f[2], f[3], None))


# ---- the clip form --------------------------------------------------------------------------------------------------
def _yuv_clip(nframes, seed=80):
    """YUV 4:2:0 of 46 x 70"""
    shapes = [(46, 70), (23, 35), (23, 35)]
    planes = [correlated(seed + k, s, nframes) for k, s in enumerate(shapes)]
    return [[planes[k][f] for k in range(3)] for f in range(nframes)]


@pytest.mark.parametrize("nframes", [1, 2, 3, 6])
@pytest.mark.parametrize("tthr2", [0, 8])
def test_clip_form(dev, nframes, tthr2):
    clip = _yuv_clip(nframes)
    frames = [_up(dev, f) for f in clip]
    dsts = [[dev.empty(p.shape[0], p.shape[1], np.uint8) for p in f] for f in clip]
    dev.probe_enable(True)
    try:
        dev.checkmate_clip(frames, dsts, 12, 12, tthr2)
        assert dev.probe_read()[1] == 1  # one launch over all planes of the clip
    finally:
        dev.probe_enable(False)
    want = ck.checkmate_clip(clip, 12, 12, tthr2)
    for f in range(nframes):
        for k in range(3):
            assert np.array_equal(dev.download(dsts[f][k]), want[f][k]), (f, k)
    for f, fr in enumerate(frames):  # the clip itself is untouched
        for k in range(3):
            assert np.array_equal(dev.download(fr[k]), clip[f][k])


# ---- tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,launches", [(128, 1), (129, 2), (300, 3)])
def test_tables_longer_than_one_launch(dev, n, launches):
    """kCheckPlanes = 128 entries per launch"""
    sets = [tuple(correlated(300 + i, (9 + i % 7, 17 + i % 37))) for i in range(n)]
    cols = [_up(dev, [s[k] for s in sets]) for k in range(5)]
    dd = [dev.empty(s[2].shape[0], s[2].shape[1], np.uint8) for s in sets]
    dev.probe_enable(True)
    try:
        for tthr2 in (0, 8):
            dev.checkmate(cols[2], dd, cols[1], cols[3], cols[0], cols[4], tthr2=tthr2)
            assert dev.probe_read()[1] == launches
            for s, d in zip(sets, dd):
                assert np.array_equal(dev.download(d), ck.checkmate(*s, tthr2=tthr2))
    finally:
        dev.probe_enable(False)


@pytest.mark.parametrize("tthr2", [0, 8])
def test_full_size(dev, tthr2):
    """three 1080 x 1920 frames, the middle one filtered"""
    shape = (1080, 1920)
    nat = fx.tiled_natural(shape, np.uint8)
    wobble = [fx.splitmix64_plane(90 + k, shape, np.uint8).astype(np.int32) % 13 - 6 for k in range(3)]
    f = [np.clip(nat.astype(np.int32) + wb, 0, 255).astype(np.uint8) for wb in wobble]
    _check(dev, [(f[0], f[0], f[1], f[2], f[2])], thr=12, tmax=12, tthr2=tthr2)


def test_prepared_form_equals_the_plain_one(dev):
    sets = [tuple(correlated(400 + i, (20 + 16 * i, 50 + 31 * i))) for i in range(4)]
    cols = [_up(dev, [s[k] for s in sets]) for k in range(5)]
    d1 = [dev.empty(s[2].shape[0], s[2].shape[1], np.uint8) for s in sets]
    d2 = [dev.empty(s[2].shape[0], s[2].shape[1], np.uint8) for s in sets]
    for tthr2 in (0, 8):
        dev.checkmate(cols[2], d1, cols[1], cols[3], cols[0], cols[4], 14, 11, tthr2)
        run = dev.prepared_checkmate(cols[2], d2, cols[1], cols[3], cols[0], cols[4], 14, 11, tthr2)
        for _ in range(3):
            run()
        for s, a, b in zip(sets, d1, d2):
            got = dev.download(a)
            assert np.array_equal(got, dev.download(b)) and np.array_equal(got, ck.checkmate(*s, 14, 11, tthr2))


def test_defaults(dev):
    f = correlated(51, (64, 200))
    d = _up(dev, f)
    o = dev.empty(64, 200, np.uint8)
    dev.checkmate([d[2]], [o], [d[1]], [d[3]])
    assert np.array_equal(dev.download(o), ck.checkmate(None, f[1], f[2], f[3], None, 12, 12, 0))


# ---- validation -----------------------------------------------------------------------------------------------------
def test_validation(dev):
    from vszip_amd import capi

    y = dev.upload(np.full((8, 64), 100, np.uint8))
    u = dev.upload(np.full((4, 32), 100, np.uint8))  # the chroma of an 8-row YUV420 clip: too short
    thin = dev.upload(np.full((8, 2), 100, np.uint8))
    o = dev.empty(8, 64, np.uint8)

    def call(srcs, dsts, thr, tmax, tthr2, nbrs=None):
        nbrs = nbrs if nbrs is not None else dev.temporal_nbrs(srcs, srcs, srcs, srcs)
        rc = dev.lib.vszip_checkmate(dev.ctx, dev.plane_table(srcs, dsts), nbrs, len(srcs), thr, tmax, tthr2)
        return rc, dev.lib.vszip_last_error(dev.ctx).decode()

    tmax_text = "Checkmate: tmax value should be in range [1;255]."
    tthr2_text = "Checkmate: tthr2 should be non-negative."
    thr_text = "Checkmate: thr value should be in range [0;255]."
    size_text = "Checkmate: clip too small; every plane must be at least 3 wide and 5 tall."
    for args, text in (((12, 0, 0), tmax_text), ((12, 256, 0), tmax_text), ((12, 12, -1), tthr2_text), ((-1, 12, 0), thr_text), ((256, 12, 0), thr_text),
                       ((-1, 0, -1), tmax_text), ((-1, 12, -1), tthr2_text)):  # ... and the order of the checks
        assert call([y], [o], *args) == (capi.ERR_ARG, text), args
    assert call([y, u], [o, u], 12, 12, 0) == (capi.ERR_ARG, size_text)
    assert call([y, thin], [o, thin], 12, 12, 4) == (capi.ERR_ARG, size_text)
    assert call([y, u], [o, u], 300, 12, 0) == (capi.ERR_ARG, thr_text)  # the parameters before the sizes
    with pytest.raises(capi.VszipError, match="tmax value should be in range") as e:
        dev.checkmate([y], [o], [y], [y], tmax=0)
    assert e.value.code == capi.ERR_ARG
    for field in ("src", "dst"):
        bad = dev.plane_table([y], [o])
        setattr(bad[0], field, None)
        rc = dev.lib.vszip_checkmate(dev.ctx, bad, dev.temporal_nbrs([y], [y]), 1, 12, 12, 0)
        assert rc == capi.ERR_ARG and "src and dst must not be NULL" in dev.lib.vszip_last_error(dev.ctx).decode()
    for field in ("p1", "n1"):
        nb = dev.temporal_nbrs([y], [y], [y], [y])
        setattr(nb[0], field, None)
        rc, msg = call([y], [o], 12, 12, 0, nb)
        assert rc == capi.ERR_ARG and "p1 and n1" in msg and "must not be NULL" in msg
    for field in ("p2", "n2"):
        nb = dev.temporal_nbrs([y], [y], [y], [y])
        setattr(nb[0], field, None)
        rc, msg = call([y], [o], 12, 12, 4, nb)
        assert rc == capi.ERR_ARG and "p2 and n2" in msg and "must not be NULL when tthr2 > 0" in msg
        assert call([y], [o], 12, 12, 0, nb)[0] == capi.OK  # ... and is not needed without tthr2
    with pytest.raises(capi.VszipError, match="must not be NULL when tthr2 > 0"):
        dev.checkmate([y], [o], [y], [y], None, None, tthr2=4)
    five = dev.upload(np.full((5, 3), 100, np.uint8))  # exactly 5 x 3 is accepted
    o5 = dev.empty(5, 3, np.uint8)
    assert call([five], [o5], 0, 1, 0)[0] == capi.OK and call([five], [o5], 255, 255, 1 << 30)[0] == capi.OK
    dev.sync()
