"""GPU: vszip_bilateral_dither against the numpy spec (tests/bilateral_dither_ref.py), bit for bit in all three sample types and on both
paths forced (VSZIP_BILATERAL_DITHER_PATH): the dense window and the sub-sampled lists (spirals and void-and-cluster scans), planes of
several tiles and of less than one, widths that are no multiple of 4, more than 23 rows and more than 23 groups, a plane as small as its
radius, radius 2, `ref` given, equal to src and absent, 10 / 12 / 16 bits with the clamp deciding, float planes around zero, per-plane
parameters, a radius whose tile does not fit, 200 planes in one call, unaligned bases and odd pitches, and the argument errors. The point
lists come from the spec; tests/test_bilateral_dither_ref.py shows the library's generator makes the same bytes, and that these inputs
take every branch of the weight."""
from functools import lru_cache

import numpy as np
import pytest

import bilateral_dither_ref as bd
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu

AUTO, TILE, DIRECT = 0, 1, 2
DTYPES = [np.uint8, np.uint16, np.float32]
IDS = ["u8", "u16", "f32"]
SIZES = [(45, 203), (131, 97), (16, 16)]
F = np.float32


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def bits_of(dtype):
    return 32 if np.dtype(dtype) == np.float32 else 8 * np.dtype(dtype).itemsize


def item(src, radius=8, thr=8.0, flat=0.4, wmin=0.1, subspl=2.0, ref=None, bits=None):
    """one plane with its wrapper arguments resolved by the spec"""
    b = bits or bits_of(src.dtype)
    d = bd.derive(src.dtype == np.float32, b, radius, thr, flat, wmin, subspl)
    return dict(src=src, ref=ref, radius=radius, bits=b, d=d, pts=bd.point_lists(radius, float(F(subspl))) if d["subsampled"] else None)


@lru_cache(maxsize=None)
def _expected(key):
    it = _expected.items[key]
    return bd.plane(it["src"], it["radius"], it["d"]["m"], it["d"]["wmax"], it["d"]["sum_w_min"], it["bits"], it["pts"], it["ref"])


_expected.items = {}


def expected(it):
    """the spec's output, computed once per (plane, ref, parameters)"""
    key = (id(it["src"]), id(it["ref"]), it["radius"], it["bits"], it["d"]["m"].tobytes(), it["d"]["wmax"].tobytes(), it["d"]["sum_w_min"].tobytes(), it["d"]["K"])
    _expected.items.setdefault(key, it)
    return _expected(key)


def run(dev, items, path=AUTO):
    up = {}

    def resident(a):
        if id(a) not in up:
            up[id(a)] = dev.upload(a) if a.ndim == 2 else dev.upload_bilateral_dither_points(a)
        return up[id(a)]
    srcs = [resident(it["src"]) for it in items]
    refs = [resident(it["ref"]) if it["ref"] is not None else None for it in items]
    dsts = [dev.empty(it["src"].shape[0], it["src"].shape[1], it["src"].dtype) for it in items]
    entries = [dev.bilateral_dither_entry(it["radius"], it["d"]["m"], it["d"]["wmax"], it["d"]["sum_w_min"], resident(it["pts"]) if it["pts"] is not None else None, it["d"]["K"])
               for it in items]
    with dev.options(VSZIP_BILATERAL_DITHER_PATH=path):
        dev.bilateral_dither(srcs, dsts, entries, refs if any(r is not None for r in refs) else None, items[0]["bits"])
    return [dev.download(d) for d in dsts]


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def check(dev, items, path=AUTO):
    outs = run(dev, items, path)
    for i, (it, o) in enumerate(zip(items, outs)):
        e = expected(it)
        assert same(o, e), (i, it["src"].shape, it["radius"], it["d"], path, int((o != e).sum()))
    return outs


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
@pytest.mark.parametrize("subspl", [2.0, 0.0, 8.0, 4.0], ids=["dense", "subspl0-K14", "subspl8-K28", "subspl4-K56-vnc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_paths_and_point_lists(dev, dtype, subspl, path):
    items = [item(bd.noisy_plane(3 + 3 * k, h, w, dtype), subspl=subspl) for k, (h, w) in enumerate(SIZES)]
    assert (items[0]["pts"] is None) == (subspl == 2.0) and items[0]["d"]["K"] == {2.0: 0, 0.0: 14, 8.0: 28, 4.0: 56}[subspl]
    check(dev, items, path)


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plane_as_small_as_its_radius_and_radius_2(dev, dtype, path):
    small = bd.noisy_plane(5, 16, 16, dtype)
    check(dev, [item(small, radius=16, subspl=2.0), item(small, radius=16, subspl=0.0), item(bd.noisy_plane(6, 16, 40, dtype), radius=16, subspl=0.0),
                item(bd.noisy_plane(7, 40, 16, dtype), radius=16, subspl=2.0)], path)
    tiny = bd.noisy_plane(8, 9, 11, dtype)
    check(dev, [item(tiny, radius=2, subspl=2.0), item(tiny, radius=2, subspl=0.0), item(tiny, radius=2, subspl=4096.0)], path)


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ref_another_plane_ref_equal_to_src_and_no_ref(dev, dtype, path):
    h, w = 45, 203
    src, other = bd.noisy_plane(3, h, w, dtype), bd.noisy_plane(4, h, w, dtype)
    for subspl in (2.0, 0.0):
        outs = check(dev, [item(src, subspl=subspl, ref=other), item(src, subspl=subspl)], path)
        assert not same(outs[0], outs[1])
        # the very src pointer as ref: the bits of ref == NULL
        s, o = dev.upload(src), dev.empty(h, w, dtype)
        it = item(src, subspl=subspl)
        pts = dev.upload_bilateral_dither_points(it["pts"]) if it["pts"] is not None else None
        with dev.options(VSZIP_BILATERAL_DITHER_PATH=path):
            dev.bilateral_dither([s], [o], [dev.bilateral_dither_entry(8, it["d"]["m"], it["d"]["wmax"], it["d"]["sum_w_min"], pts, it["d"]["K"])], [s], it["bits"])
        assert same(dev.download(o), outs[1])


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
@pytest.mark.parametrize("bits", [10, 12, 16])
def test_u16_depths_and_the_clamp(dev, bits, path):
    """the 16-bit plane scaled to the depth; and samples from a few units under 2^bits - 1 to three above it (a host may pass such) with a large
    thr, so that every tap counts and the mean of a neighbourhood above the peak is brought back by the clamp"""
    peak = (1 << bits) - 1
    h, w = 45, 203
    base = (bd.noisy_plane(3, h, w, np.uint16).astype(np.uint32) * (peak + 1) >> 16).astype(np.uint16)
    high = np.minimum(peak + 3 - (base.astype(np.uint32) >> (bits - 4)), 65535).astype(np.uint16)
    for a in (base, high):
        a.setflags(write=False)
    items = [item(base, bits=bits), item(base, bits=bits, subspl=0.0), item(high, bits=bits, thr=200.0, flat=0.0), item(high, bits=bits, thr=200.0, subspl=8.0)]
    outs = check(dev, items, path)
    if bits < 16:
        assert high.max() > peak and outs[2].max() <= peak and outs[3].max() <= peak and (outs[2] == peak).any()


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
def test_float_planes_around_zero(dev, path):
    planes = [np.ascontiguousarray(bd.noisy_plane(3 + 3 * k, h, w, np.float32) * F(2.2) - F(0.5)) for k, (h, w) in enumerate(SIZES[:2])]
    assert all(-0.5 <= p.min() < -0.3 and 0.3 < p.max() <= 0.5 for p in planes)
    check(dev, [item(p, subspl=s) for p in planes for s in (2.0, 0.0)], path)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_per_plane_parameters_differ_within_a_call(dev, dtype):
    src = bd.noisy_plane(6, 131, 97, dtype)
    items = [item(src), item(src, radius=4), item(src, thr=24.0, flat=0.0), item(src, wmin=4.0), item(src, subspl=0.0), item(src, radius=12, subspl=16.0)]
    for path in (TILE, DIRECT):
        outs = check(dev, items, path)
        assert all(not same(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("path", [AUTO, TILE], ids=["auto", "tile-does-not-fit"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_radius_40_goes_the_direct_path(dev, dtype, path):
    """the tile plus a 39-sample halo is beyond the tile path's LDS budget: auto takes the direct path, a forced tile falls back"""
    src = bd.noisy_plane(3, 45, 203, dtype)
    sub = item(src, radius=40, subspl=0.0)
    assert sub["d"]["K"] == 78
    check(dev, [item(src, radius=40, subspl=2.0), sub], path)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_200_small_planes_in_one_call(dev, dtype):
    """three launches of the 96-entry table; dense and sub-sampled planes alternate in runs, so the launches are cut by kind too"""
    sizes = [(8 + i % 11, 8 + i % 37) for i in range(200)]
    check(dev, [item(bd.noisy_plane(i % 7, h, w, dtype), radius=4 + 4 * (i // 50 % 2), subspl=2.0 if i // 25 % 2 else 0.0) for i, (h, w) in enumerate(sizes)])


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_bases_and_odd_pitches_give_the_same_bits(dev, dtype, path):
    """every pointer one element off a 16-byte boundary and every pitch odd, each in turn and all together"""
    h, w = 45, 203
    keep = []

    def shifted(a, shift, pitch):
        a = np.ascontiguousarray(a)
        big = dev.empty(a.shape[0] + 1, pitch + 32, a.dtype)
        keep.append(big)
        v = dev.wrap(big.ptr + shift * a.itemsize, a.shape[0], a.shape[1], pitch, a.dtype)
        dev.copy_in(v, a)
        dev.sync()
        return v
    src, other = bd.noisy_plane(3, h, w, dtype), bd.noisy_plane(4, h, w, dtype)
    for subspl in (2.0, 0.0):
        it = item(src, subspl=subspl, ref=other)
        want = expected(it)
        for which in ("src", "ref", "dst", "points", "all"):
            on = lambda k: which in (k, "all")
            s = shifted(src, 1 if on("src") else 0, 211 if on("src") else 224)
            r = shifted(other, 1 if on("ref") else 0, 209 if on("ref") else 224)
            d = dev.wrap(shifted(np.zeros_like(src), 1 if on("dst") else 0, 213 if on("dst") else 224).ptr, h, w, 213 if on("dst") else 224, dtype)
            pts = None
            if it["pts"] is not None:
                flat = np.ascontiguousarray(it["pts"]).reshape(1, -1)
                pts = shifted(flat, 1 if on("points") else 0, flat.shape[1] + 3)  # (one int16 off: the pairs are 2-byte aligned only)
            e = dev.bilateral_dither_entry(8, it["d"]["m"], it["d"]["wmax"], it["d"]["sum_w_min"], pts, it["d"]["K"])
            with dev.options(VSZIP_BILATERAL_DITHER_PATH=path):
                dev.bilateral_dither([s], [d], [e], [r], it["bits"])
            assert same(dev.download(d), want), (subspl, which)
    dev.sync()


def test_argument_errors(dev):
    src = dev.upload(np.zeros((20, 20), np.uint16))
    dst = dev.empty(20, 20, np.uint16)
    pts = dev.upload_bilateral_dither_points(bd.point_lists(8, 0.0))
    E = dev.bilateral_dither_entry
    for entries, kw, code, msg in [
        ([E(24, 1, 1, 1)], {}, -1, 'BilateralDither: picture size must be greater than "radius"'),
        ([E(1, 1, 1, 1)], {}, -1, "radius 1 is outside 2..16384"),
        ([E(16385, 1, 1, 1)], {}, -1, "radius 16385 is outside 2..16384"),
        ([E(8, 1, 1, 1, None, 14)], {}, -1, "needs its point lists"),
        ([E(8, 1, 1, 1, pts, 2)], {}, -1, "K = 2 is outside 3..4096"),
        ([E(8, 1, 1, 1)], dict(bits=8), -1, "bits per sample"),
        ([E(8, 1, 1, 1)], dict(bits=17), -1, "bits per sample"),
    ]:
        with pytest.raises(VszipError, match=msg) as ei:
            dev.bilateral_dither([src], [dst], entries, **kw)
        assert ei.value.code == code
    with pytest.raises(VszipError, match="dst must not overlap an input"):
        dev.bilateral_dither([src], [src], [E(8, 1, 1, 1)])
    big = dev.upload(np.zeros((130, 130), np.uint16))
    with pytest.raises(VszipError, match="the dense window serves radius <= 128") as ei:
        dev.bilateral_dither([big], [dev.empty(130, 130, np.uint16)], [E(129, 1, 1, 1)])
    assert ei.value.code == -3
    s16 = dev.upload(np.zeros((8, 8), np.float16))
    with pytest.raises(VszipError, match="8..16-bit integer or 32-bit float"):
        dev.bilateral_dither([s16], [dev.empty(8, 8, np.float16)], [E(2, 1, 1, 1)])
    dev.bilateral_dither([src], [dst], [E(8, 1, 1, 1, pts, 14)])  # and the valid call goes through
    dev.bilateral_dither([src], [dst], [E(8, 1, 1, 1)])
    assert not dev.download(dst).any()
