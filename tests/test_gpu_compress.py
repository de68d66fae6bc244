"""GPU: vszip_compress against the numpy spec (tests/compress_ref.py), bit for bit: planes of less than a block, of exactly one, of
partial blocks in either direction and of more than one workgroup, in one call and alone; every parameter set of both codecs; luma and
chroma tables mixed in one call; 200 planes in one call; dst == src; unaligned bases and odd pitches; the reference's golden inputs
through the device; and the argument errors. tests/test_compress_ref.py shows that these inputs take every branch of the pipeline and
that the library's table generator equals the spec's; tests/test_compress_block_host.py runs the block body on the host."""
from functools import lru_cache

import numpy as np
import pytest

import compress_ref as cr
import fixtures as fx
from vszip_amd import capi
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu

PARAMS = cr.MPEG2_PARAMS + cr.JPEG_PARAMS
IDS = [",".join(f"{k}={v}" for k, v in kw.items()) for kw in PARAMS]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _key(kw):
    return tuple(sorted(dict(cr.DEFAULTS, **kw).items()))


@lru_cache(maxsize=None)
def _expected(pid, key, chroma):
    return cr.plane(_expected.planes[pid], cr.tables(**dict(key)), chroma)


_expected.planes = {}


def expected(p, kw, chroma=False):
    """the spec's output, computed once per (plane, parameters, table)"""
    _expected.planes.setdefault(id(p), p)
    return _expected(id(p), _key(kw), bool(chroma))


def lib_tables(kw):
    return capi.compress_tables(**dict(cr.DEFAULTS, **kw))


def check(dev, planes, kw, chroma=None):
    srcs = [dev.upload(p) for p in planes]
    dsts = [dev.empty(p.shape[0], p.shape[1], np.uint8) for p in planes]
    dev.compress(srcs, dsts, lib_tables(kw), chroma)
    outs = [dev.download(d) for d in dsts]
    for i, (p, o) in enumerate(zip(planes, outs)):
        e = expected(p, kw, chroma[i] if isinstance(chroma, (list, tuple)) else bool(chroma))
        assert o.dtype == e.dtype and o.shape == e.shape and np.array_equal(o, e), (i, p.shape, kw, chroma, int((o != e).sum()))
    return outs


@pytest.mark.parametrize("kw", PARAMS, ids=IDS)
def test_every_size_in_one_call(dev, kw):
    planes = cr.gpu_planes(0)
    assert [p.shape for p in planes] == [(1, 1), (13, 7), (8, 8), (9, 9), (83, 37), (72, 64), (67, 130)]
    check(dev, planes, kw)


@pytest.mark.parametrize("kw", [PARAMS[2], PARAMS[8]], ids=[IDS[2], IDS[8]])
def test_every_size_alone_and_the_other_content(dev, kw):
    for p in cr.gpu_planes(0) + cr.gpu_planes(1):
        check(dev, [p], kw)
    # more than one workgroup a plane (420 and 1 189 blocks of 256 a workgroup), behind and before other planes
    check(dev, [cr.gpu_plane(3, 9, 9), cr.gpu_plane(2, 333, 75), cr.gpu_plane(5, 325, 227), cr.gpu_plane(4, 37, 83)], kw, [False, True, False, True])


@pytest.mark.parametrize("kw", PARAMS, ids=IDS)
def test_luma_and_chroma_tables_mixed_in_one_call(dev, kw):
    planes = cr.gpu_planes(1) + cr.gpu_planes(0)
    chroma = [bool((i // 2) & 1) for i in range(len(planes))]
    outs = check(dev, planes, kw, chroma)
    check(dev, planes[4:6], kw, True)  # a scalar serves every plane
    assert chroma[3] and planes[3].shape == (9, 9)  # (noise)
    if kw["codec"] == 1 and kw["quality"] not in (1, 100):  # jpeg: the two tables differ (mpeg2: both alike; quality 1: all 255, 100: all ones)
        assert not np.array_equal(outs[3], expected(planes[3], kw, False))
    else:
        assert np.array_equal(outs[3], expected(planes[3], kw, False))


@pytest.mark.parametrize("kw", [PARAMS[2], PARAMS[8]], ids=[IDS[2], IDS[8]])
def test_200_planes_in_one_call(dev, kw):
    """two launches: the table holds 192 planes"""
    sizes = [(1 + i % 19, 1 + i % 37) for i in range(200)]
    planes = [cr.gpu_plane(i % 6, w, h) for i, (h, w) in enumerate(sizes)]
    check(dev, planes, kw, [bool(i % 3) for i in range(200)])


@pytest.mark.parametrize("kw", [PARAMS[0], PARAMS[5], PARAMS[7], PARAMS[9]], ids=[IDS[0], IDS[5], IDS[7], IDS[9]])
def test_in_place_equals_out_of_place(dev, kw):
    planes = cr.gpu_planes(0)
    bufs = [dev.upload(p) for p in planes]
    dev.compress(bufs, bufs, lib_tables(kw))
    for p, b in zip(planes, bufs):
        assert np.array_equal(dev.download(b), expected(p, kw)), p.shape


@pytest.mark.parametrize("kw", [PARAMS[2], PARAMS[8]], ids=[IDS[2], IDS[8]])
def test_unaligned_bases_and_odd_pitches_give_the_same_bits(dev, kw):
    """base offsets of 1 .. 7 bytes and odd pitches, on the source, the destination and both; and 8-byte aligned with a pitch of 8 k"""
    keep = []

    def shifted(a, shift, pitch):
        big = dev.empty(a.shape[0] + 1, pitch + 32, np.uint8)
        keep.append(big)
        v = dev.wrap(big.ptr + shift, a.shape[0], a.shape[1], pitch, np.uint8)
        dev.copy_in(v, np.ascontiguousarray(a))
        return v
    tb = lib_tables(kw)
    for p in (cr.gpu_plane(4, 37, 83), cr.gpu_plane(6, 130, 67)):
        h, w = p.shape
        want, zeros = expected(p, kw), np.zeros_like(p)
        for shift in range(8):
            for which in ("src", "dst", "both"):
                s = shifted(p, shift if which != "dst" else 0, w + 3 + 2 * shift if which != "dst" else 136)
                d = shifted(zeros, shift if which != "src" else 0, w + 5 + 2 * shift if which != "src" else 136)
                dev.compress([s], [d], tb)
                assert np.array_equal(dev.download(d), want), (p.shape, shift, which)
        s, d = shifted(p, 8, 136), shifted(zeros, 16, 144)
        dev.compress([s], [d], tb)
        assert np.array_equal(dev.download(d), want)
    dev.sync()


@pytest.mark.parametrize("fmt", ["GRAY8", "YUV420P8"])
def test_golden_inputs_through_the_device_give_the_golden_stats(dev, fmt):
    planes = cr.golden_inputs(fmt, "full")
    assert planes[0].shape == (320, 640)
    keys = [k for k in sorted(cr.goldens()) if cr.parse_key(k)[:2] == (fmt, "full")]
    assert len(keys) == (12 if fmt == "GRAY8" else 4)
    srcs = [dev.upload(p) for p in planes]
    for key in keys:
        kw = cr.parse_key(key)[2]
        with_chroma = kw.pop("chroma", True)
        n = len(planes) if with_chroma else 1
        dsts = [dev.empty(p.shape[0], p.shape[1], np.uint8) for p in planes[:n]]
        dev.compress(srcs[:n], dsts, lib_tables(kw), [i != 0 for i in range(n)])
        outs = [dev.download(d) for d in dsts] + [p.copy() for p in planes[n:]]  # planes the wrapper does not process are the host's copy
        assert all(np.array_equal(o, e) for o, e in zip(outs, cr.run_key(key))), key  # (13 and 4 workgroups a plane)
        for i, o in enumerate(outs):
            st, g = fx.plane_stats(o), cr.goldens()[key][f"p{i}"]
            assert st["min"] == g["min"] and st["max"] == g["max"] and st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i, st, g)


def test_the_tables_are_consumed_before_the_call_returns(dev):
    p, kw = cr.gpu_plane(4, 130, 67), PARAMS[2]
    s, d = dev.upload(p), dev.empty(67, 130, np.uint8)
    tb = lib_tables(kw)
    dev.compress([s], [d], tb)
    for i in range(64):  # overwritten at once, before the stream is drained
        tb.qmul[0][i] = tb.deq[0][i] = 0
    tb.dc_q = tb.dc_scale = 1
    assert np.array_equal(dev.download(d), expected(p, kw))


def test_argument_errors(dev):
    src, dst = dev.upload(np.zeros((20, 20), np.uint8)), dev.empty(20, 20, np.uint8)
    tb = lib_tables(PARAMS[2])
    with pytest.raises(VszipError, match="Compress: tables must not be NULL") as ei:
        dev.compress([src], [dst], None)
    assert ei.value.code == -1
    for codec in (-1, 2):
        bad = lib_tables(PARAMS[2])
        bad.codec = codec
        with pytest.raises(VszipError, match=r"Compress: codec must be 0 \(mpeg2\) or 1 \(jpeg\)\.") as ei:
            dev.compress([src], [dst], bad)
        assert ei.value.code == -1
    bad = lib_tables(PARAMS[2])
    bad.dc_q = 0
    with pytest.raises(VszipError, match="Compress: dc_q must be positive") as ei:
        dev.compress([src], [dst], bad)
    assert ei.value.code == -1
    for field, value in (("qmul", -1), ("qmul", (1 << 20) + 1), ("deq", -1), ("deq", 1 << 15)):
        bad = lib_tables(PARAMS[8])
        getattr(bad, field)[1][63] = value
        with pytest.raises(VszipError, match=r"Compress: tables: qmul\[1\]\[63\] = -?\d+, deq = -?\d+ are outside 0..1048576, 0..32767") as ei:
            dev.compress([src], [dst], bad)
        assert ei.value.code == -1
    for s, d in ((dev.wrap(0, 20, 20, 20, np.uint8), dst), (src, dev.wrap(0, 20, 20, 20, np.uint8))):
        with pytest.raises(VszipError, match="Compress: plane 1: src and dst must not be NULL") as ei:
            dev.compress([src, s], [dst, d], tb)
        assert ei.value.code == -1
    with pytest.raises(VszipError, match=r"Compress: plane 0: bad geometry 20x20, pitches 16 / \d+") as ei:
        dev.compress([dev.wrap(src.ptr, 20, 20, 16, np.uint8)], [dst], tb)
    assert ei.value.code == -1
    with pytest.raises(ValueError, match="8-bit planes only"):
        dev.compress([dev.upload(np.zeros((8, 8), np.uint16))], [dev.empty(8, 8, np.uint16)], tb)
    dev.compress([src], [dst], tb)  # and the valid call goes through: a black plane stays black
    assert not dev.download(dst).any()
