"""GPU parity: vszip_mosquito_nr vs the CPU restatement (tests/mosquito_ref.py), bit for bit in all three sample types,
float included: the reference's goldens (all 22 keys), every size from 4 x 4 to 12 x 12 in one call, the tile seams,
the parameter grid, per-plane parameters in one call, the bit depths, the float clamps, the input that reaches both
output clamps, unaligned layouts, the prepared form and the create-time errors."""
import itertools

import numpy as np
import pytest

import fixtures as fx
import mosquito_ref as mq

pytestmark = pytest.mark.gpu

TW, TH = 64, 32  # kTW, kTH of csrc/mosquito_nr.hip: the outputs of a workgroup

DTYPES = [(np.uint8, 8), (np.uint16, 16), (np.float32, 32)]
IDS = ["u8", "u16", "f32"]
RESTORES = [0, 1, 64, 127, 128]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def noise(seed, shape, dtype, bits=None):
    """full-range integers (of `bits`), floats in [-0.2, 1.2)"""
    a = fx.splitmix64_plane(seed, shape, dtype)
    if np.dtype(dtype) == np.float32:
        return (a * np.float32(1.4) - np.float32(0.2)).astype(np.float32)
    return (a >> (8 * a.itemsize - bits)).astype(dtype) if bits else a


def binary_noise(seed, shape, dtype, bits):
    """independent samples of 0 or the peak: the output reaches both clamps (tests/test_mosquito_ref.py)"""
    m = fx.splitmix64_plane(seed, shape, np.uint8) & 1
    return m.astype(np.float32) if np.dtype(dtype) == np.float32 else (m.astype(np.int64) * ((1 << bits) - 1)).astype(dtype)


def natural(shape, dtype, bits):
    a = fx.tiled_natural(shape, dtype)
    return (a >> (16 - bits)).astype(dtype) if np.dtype(dtype) == np.uint16 and bits < 16 else a


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want):
    """bit for bit (a float +0 is not a -0)"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(np.ascontiguousarray(want)))


def _run(dev, planes, strength, restore, radius, bits, chroma=None, align=32):
    ss = [dev.upload(np.ascontiguousarray(p), align) for p in planes]
    dd = [dev.empty(p.shape[0], p.shape[1], p.dtype, align) for p in planes]
    dev.mosquito_nr(ss, dd, strength, restore, radius, None if planes[0].dtype == np.float32 else bits, chroma)
    return [dev.download(d) for d in dd]


def _per(v, n):
    return [v] * n if isinstance(v, (int, bool)) or v is None else list(v)


def _check(dev, planes, strength, restore, radius, bits, chroma=None, align=32):
    n = len(planes)
    got = _run(dev, planes, strength, restore, radius, bits, chroma, align)
    st, rs, rd, ch = _per(strength, n), _per(restore, n), _per(radius, n), _per(chroma, n)
    for i, (p, g) in enumerate(zip(planes, got)):
        want = mq.mosquito_nr(p, st[i], rs[i], rd[i], None if p.dtype == np.float32 else bits, bool(ch[i]))
        assert _same(g, want), (i, p.shape, p.dtype, st[i], rs[i], rd[i], ch[i], int((_bits(g) != _bits(want)).sum()), np.argwhere(_bits(g) != _bits(want))[:4].tolist())


# ---- goldens --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(mq.goldens()))
def test_reference_goldens(dev, key):
    fmt, geometry, kw = mq.parse_key(key)
    bits = mq.format_bits(fmt)
    planes = mq.golden_inputs(fmt, geometry)
    which = kw["which"]
    st, rs, rd = mq.check_mosquito_args([planes[k].shape for k in which], kw.get("strength", 16), kw.get("restore", 128), kw.get("radius", 2))
    # one call over the processed planes, each with its slot's parameters; the others are the wrapper's copies
    got = _run(dev, [planes[k] for k in which], [st[k] for k in which], [rs[k] for k in which], [rd[k] for k in which], bits, [k > 0 for k in which])
    outs = [p.copy() for p in planes]
    for k, g in zip(which, got):
        outs[k] = g
    for i, (g, w) in enumerate(zip(outs, mq.run_key(key))):
        assert _same(g, w), (key, i)
        s, gold = mq.golden_stats(g, bits), mq.goldens()[key][f"p{i}"]
        if g.dtype.kind == "f":
            assert s["min"] == pytest.approx(gold["min"], abs=1e-7, rel=0) and s["max"] == pytest.approx(gold["max"], abs=1e-7, rel=0), (key, i)
        else:
            assert s["min"] == gold["min"] and s["max"] == gold["max"], (key, i)
        assert s["avg"] == pytest.approx(gold["avg"], rel=1e-9, abs=0), (key, i)


# ---- sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bits", DTYPES, ids=IDS)
def test_every_small_size_in_one_call(dev, dtype, bits):
    """4 .. 12 x 4 .. 12: 81 planes, radius and restore cycling; reflection, the n - 2 rule, odd and even lifting lengths"""
    sizes = list(itertools.product(range(4, 13), range(4, 13)))
    planes = [noise(10 + i, (h, w), dtype) if i % 3 else binary_noise(i, (h, w), dtype, bits) for i, (w, h) in enumerate(sizes)]
    n = len(planes)
    assert n == 81
    _check(dev, planes, [(1, 16, 32, 7)[i % 4] for i in range(n)], [RESTORES[i % 5] for i in range(n)], [1 + i % 2 for i in range(n)], bits, [i % 2 == 1 for i in range(n)])
    _check(dev, planes, 16, [RESTORES[(i + 2) % 5] for i in range(n)], [2 - i % 2 for i in range(n)], bits)


@pytest.mark.parametrize("dtype,bits", DTYPES, ids=IDS)
@pytest.mark.parametrize("content", ["noise", "natural"])
def test_tile_edge_sizes(dev, dtype, bits, content):
    sizes = list(itertools.product((TW - 1, TW, TW + 1, 2 * TW + 3), (TH - 1, TH, TH + 1, 2 * TH + 3)))
    make = (lambda i, s: noise(200 + i, s, dtype)) if content == "noise" else (lambda i, s: natural(s, dtype, bits))
    planes = [make(i, (h, w)) for i, (w, h) in enumerate(sizes)]
    n = len(planes)
    for radius in (1, 2):
        _check(dev, planes, 16, [RESTORES[(i + i // 4 + radius) % 5] for i in range(n)], radius, bits)


@pytest.mark.parametrize("dtype,bits", DTYPES, ids=IDS)
@pytest.mark.parametrize("radius", [1, 2])
def test_parameter_grid(dev, dtype, bits, radius):
    """strength x restore on one odd-sized plane of several tiles: 20 planes a call"""
    a = noise(31, (2 * TH + 5, 2 * TW + 7), dtype)
    grid = list(itertools.product((0, 1, 16, 32), RESTORES))
    _check(dev, [a] * len(grid), [g[0] for g in grid], [g[1] for g in grid], radius, bits)


@pytest.mark.parametrize("dtype,bits", DTYPES, ids=IDS)
def test_mixed_parameters_in_one_call(dev, dtype, bits):
    shapes = [(45, 203), (22, 101), (22, 101), (4, 4), (70, 66), (33, 130)]
    planes = [noise(40 + i, s, dtype) for i, s in enumerate(shapes)]
    _check(dev, planes, [16, 0, 8, 32, 0, 24], [128, 64, 0, 127, 128, 96], [2, 1, 1, 2, 2, 1], bits, [False, True, True, False, True, False])
    srcs = [dev.upload(p) for p in planes]  # the sources are inputs only
    dsts = [dev.empty(p.shape[0], p.shape[1], p.dtype) for p in planes]
    dev.mosquito_nr(srcs, dsts, [16, 0, 8, 32, 0, 24], 128, 2, None if bits == 32 else bits)
    assert all(_same(dev.download(s), p) for s, p in zip(srcs, planes))
    assert _same(dev.download(dsts[1]), planes[1]) and _same(dev.download(dsts[4]), planes[4])  # strength 0: copies


# ---- bit depths, clamps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [9, 10, 12, 14, 16])
def test_bit_depths(dev, bits):
    shape = (TH + 7, TW + 9)
    planes = [noise(50, shape, np.uint16, bits), binary_noise(51, shape, np.uint16, bits), natural(shape, np.uint16, bits)]
    assert planes[0].max() <= (1 << bits) - 1
    for radius, restore in ((2, 128), (1, 64)):
        _check(dev, planes, 32, restore, radius, bits)


def test_samples_above_the_peak_are_processed_and_clamped(dev):
    """a 10-bit call on full-range 16-bit samples: no error, the reference's arithmetic, the result clamped to 1023"""
    a = noise(52, (TH + 7, TW + 9), np.uint16)
    assert a.max() > 60000
    for radius, restore in ((2, 128), (1, 64), (2, 0)):
        _check(dev, [a], 16, restore, radius, 10)
    assert _run(dev, [a], 16, 128, 2, 10)[0].max() == 1023


@pytest.mark.parametrize("dtype,bits", [(np.uint8, 8), (np.uint16, 10), (np.uint16, 16), (np.float32, 32)], ids=["u8", "u10", "u16", "f32"])
def test_binary_noise_reaches_both_clamps(dev, dtype, bits):
    a = binary_noise(5, (64, 66), dtype, bits)
    _check(dev, [a, a, a], 32, [128, 127, 0], [2, 2, 1], bits)
    out = _run(dev, [a], 32, 128, 2, bits)[0]
    assert out.min() == 0 and out.max() == (1.0 if bits == 32 else (1 << bits) - 1)


def test_float_clamps_and_flat_planes(dev):
    shape = (TH + 3, TW + 5)
    wide = (fx.splitmix64_plane(60, shape, np.float32) * np.float32(3) - np.float32(1)).astype(np.float32)  # [-1, 2)
    flat = np.full(shape, np.float32(0.3), np.float32)
    below = np.full(shape, np.float32(-0.75), np.float32)
    planes = [wide, wide, flat, below, below]
    chroma = [False, True, False, False, True]
    _check(dev, planes, 24, [128, 64, 128, 128, 0], [2, 1, 2, 1, 2], 32, chroma)
    got = _run(dev, planes, 24, 128, 2, 32, chroma)
    assert got[0].min() == 0.0 and got[0].max() == 1.0 and got[1].min() == -0.5 and got[1].max() == 0.5
    assert _same(got[2], flat) and (got[3] == 0.0).all() and (got[4] == -0.5).all()


# ---- layouts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bits", DTYPES, ids=IDS)
@pytest.mark.parametrize("shift", [1, 3])
def test_base_offsets_and_odd_pitches(dev, dtype, bits, shift):
    """source and destination `shift` samples into their allocations, with odd pitches: the sample-by-sample path"""
    h, w = TH + 13, TW + 75
    a = noise(70 + shift, (h, w), dtype)
    big = dev.upload(np.pad(a, ((0, 0), (shift, 2 - shift % 2))), 1)
    assert big.stride % 2 == 1
    out = dev.empty(h, big.stride + 2, dtype, 1)
    isz = np.dtype(dtype).itemsize
    src = dev.wrap(big.ptr + shift * isz, h, w, big.stride, dtype)
    dst = dev.wrap(out.ptr + shift * isz, h, w, out.stride, dtype)
    aligned = _run(dev, [a, a], [16, 0], [64, 128], 2, bits)
    for k, strength in enumerate((16, 0)):
        dev.mosquito_nr([src], [dst], strength, 64, 2, None if bits == 32 else bits)
        got = dev.download(out)[:, shift:shift + w]
        assert _same(np.ascontiguousarray(got), aligned[k]) and _same(aligned[k], mq.mosquito_nr(a, strength, 64, 2, None if bits == 32 else bits))


@pytest.mark.parametrize("align", [1, 4, 8])
def test_strides(dev, align):
    for dtype, bits in DTYPES:
        planes = [noise(80, (41, 203), dtype), noise(81, (37, 150), dtype), noise(82, (9, 131), dtype)]
        _check(dev, planes, [16, 32, 0], [128, 64, 0], [2, 1, 2], bits, None, align)


def test_one_side_unaligned(dev):
    """an aligned source with an unaligned destination and the reverse"""
    h, w = 40, 150
    a = noise(90, (h, w), np.uint8)
    want = mq.mosquito_nr(a, 16, 128, 2)
    s_al, d_al = dev.upload(a), dev.empty(h, w, np.uint8)
    big = dev.upload(np.pad(a, ((0, 0), (1, 0))))
    s_un = dev.wrap(big.ptr + 1, h, w, big.stride, np.uint8)
    obig = dev.empty(h, w + 1, np.uint8)
    d_un = dev.wrap(obig.ptr + 1, h, w, obig.stride, np.uint8)
    dev.mosquito_nr([s_un], [d_al])
    assert _same(dev.download(d_al), want)
    dev.mosquito_nr([s_al], [d_un])
    assert _same(np.ascontiguousarray(dev.download(obig)[:, 1:]), want)


# ---- forms ----------------------------------------------------------------------------------------------------------
def test_prepared_form_and_defaults(dev):
    planes = [noise(95 + i, (20 + 16 * i, 50 + 31 * i), np.uint16) for i in range(4)]
    srcs = [dev.upload(p) for p in planes]
    d1 = [dev.empty(p.shape[0], p.shape[1], p.dtype) for p in planes]
    d2 = [dev.empty(p.shape[0], p.shape[1], p.dtype) for p in planes]
    dev.mosquito_nr(srcs, d1)
    run = dev.prepared_mosquito_nr(srcs, d2)
    for _ in range(3):
        run()
    for p, a, b in zip(planes, d1, d2):
        got = dev.download(a)
        assert _same(got, dev.download(b)) and _same(got, mq.mosquito_nr(p, 16, 128, 2, 16))


def test_full_size(dev):
    """one 1080p plane a sample type: many tiles, one launch"""
    dev.probe_enable(True)
    try:
        for dtype, bits in DTYPES:
            a = natural((1080, 1920), dtype, bits)
            _check(dev, [a], 16, 128, 2, bits)
            assert dev.probe_read()[1] == 1
    finally:
        dev.probe_enable(False)


# ---- validation -----------------------------------------------------------------------------------------------------
def test_validation(dev):
    import ctypes as C

    from vszip_amd import capi

    y = dev.upload(np.full((8, 64), 100, np.uint8))
    u = dev.upload(np.full((3, 32), 100, np.uint8))
    thin = dev.upload(np.full((8, 3), 100, np.uint8))
    y16 = dev.upload(np.full((8, 64), 100, np.uint16))
    o, o16 = dev.empty(8, 64, np.uint8), dev.empty(8, 64, np.uint16)
    i32 = lambda v: (C.c_int32 * len(v))(*v)

    def call(srcs, dsts, st, rs, rd, dtype=capi.U8, bits=8, table=None):
        n = len(srcs)
        rc = dev.lib.vszip_mosquito_nr(dev.ctx, dtype, bits, table if table is not None else dev.plane_table(srcs, dsts), n,
                                       i32(st) if st is not None else None, i32(rs) if rs is not None else None, i32(rd) if rd is not None else None, None)
        return rc, dev.lib.vszip_last_error(dev.ctx).decode()

    fmt_text = "MosquitoNR: only constant-format 8..16 bit integer or 32 bit float input is supported."
    size_text = "MosquitoNR: input is too small (need at least 4x4 per processed plane)."
    for dtype, bits in ((capi.U8, 9), (capi.U8, 7), (capi.U16, 8), (capi.U16, 17), (capi.F16, 16), (4, 32)):
        assert call([y], [o], [16], [128], [2], dtype, bits) == (capi.ERR_ARG, fmt_text), (dtype, bits)
    assert call([y, u], [o, u], [16, 16], [128, 128], [2, 2]) == (capi.ERR_ARG, size_text)
    assert call([y, thin], [o, thin], [16, 16], [128, 128], [2, 2]) == (capi.ERR_ARG, size_text)
    for st, rs, rd, text in (([-1], [128], [2], "MosquitoNR: strength value -1 is below minimum 0."), ([33], [128], [2], "MosquitoNR: strength value 33 is above maximum 32."),
                             ([16], [-1], [2], "MosquitoNR: restore value -1 is below minimum 0."), ([16], [129], [2], "MosquitoNR: restore value 129 is above maximum 128."),
                             ([16], [128], [0], "MosquitoNR: radius value 0 is below minimum 1."), ([16], [128], [3], "MosquitoNR: radius value 3 is above maximum 2."),
                             ([99], [-1], [0], "MosquitoNR: strength value 99 is above maximum 32."), ([16], [-1], [0], "MosquitoNR: restore value -1 is below minimum 0.")):
        assert call([y], [o], st, rs, rd) == (capi.ERR_ARG, text), (st, rs, rd)
    # any plane's slot, and the sizes before the parameters
    assert call([y, y], [o, o], [16, 33], [128, 128], [2, 2]) == (capi.ERR_ARG, "MosquitoNR: strength value 33 is above maximum 32.")
    assert call([y, y], [o, o], [16, 16], [128, 128], [2, 0]) == (capi.ERR_ARG, "MosquitoNR: radius value 0 is below minimum 1.")
    assert call([y, u], [o, u], [99, 16], [128, 128], [2, 2]) == (capi.ERR_ARG, size_text)
    for missing in range(3):
        arrs = [[16], [128], [2]]
        arrs[missing] = None
        rc, msg = call([y], [o], *arrs)
        assert rc == capi.ERR_ARG and "must not be NULL" in msg
    for field in ("src", "dst"):
        bad = dev.plane_table([y], [o])
        setattr(bad[0], field, None)
        rc, msg = call([y], [o], [16], [128], [2], table=bad)
        assert rc == capi.ERR_ARG and "src and dst must not be NULL" in msg
    with pytest.raises(capi.VszipError, match="strength value 40 is above maximum 32") as e:
        dev.mosquito_nr([y], [o], strength=40)
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.VszipError, match="8..16 bit integer or 32 bit float"):
        dev.mosquito_nr([y16], [o16], bits=8)
    four = dev.upload(np.full((4, 4), 100, np.uint8))  # exactly 4 x 4 and every bound are accepted
    o4 = dev.empty(4, 4, np.uint8)
    for st, rs, rd in ((0, 0, 1), (32, 128, 2)):
        assert call([four], [o4], [st], [rs], [rd])[0] == capi.OK
    assert call([y16], [o16], [16], [128], [2], capi.U16, 9)[0] == capi.OK and call([y16], [o16], [16], [128], [2], capi.U16, 16)[0] == capi.OK
    dev.sync()
