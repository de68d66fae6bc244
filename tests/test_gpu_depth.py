"""GPU: vszip_depth against the numpy spec (tests/depth_ref.py), bit for bit. Error diffusion 16 -> 8, 16 -> 10, 16 -> 15 and 10 -> 8 and `none`
both ways, limited range and full range (non-chroma), on w in {1, 2, 3, 63, 64, 65, 129} x h in {1, 2, 63, 64, 65, 129, 257} (one, two and several
64-row bands; both workgroup sizes, each also forced on the other's planes), 1030 rows x 40 columns (more rows than a workgroup holds: the carry
row in LDS), rows wide enough for a band to wait for its wave, a plane wide enough for the carry row to leave LDS for the context's scratch (with a
few rows, where no carry is needed, and with enough rows under the small workgroup to use it), bases and pitches off four samples, 200 planes of
mixed sizes in one call, content that holds at 0 and at the peak for runs (the clamp feeds the error) over noise, natural content, and the same
call twice on one context."""
from functools import lru_cache

import numpy as np
import pytest

import depth_ref as dr
import fixtures as fx
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu

WS, HS = (1, 2, 3, 63, 64, 65, 129), (1, 2, 63, 64, 65, 129, 257)
SIZES = [(h, w) for h in HS for w in WS]
DIFFUSE = [(16, 8), (16, 10), (16, 15), (10, 8)]
NONE = [(8, 16), (16, 8), (10, 16), (16, 10), (8, 8), (12, 12)]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


@lru_cache(maxsize=None)
def plane(seed, h, w, bits):
    a = dr.content(seed, h, w, bits)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def want(seed, h, w, bits_in, bits_out, dither, full):
    a = dr.convert(plane(seed, h, w, bits_in), bits_in, bits_out, dither, full)
    a.setflags(write=False)
    return a


def run(dev, srcs, bits_in, bits_out, dither, full=False, **opts):
    s = [dev.upload(a) for a in srcs]
    d = [dev.empty(a.shape[0], a.shape[1], dr.dtype_of(bits_out)) for a in srcs]
    with dev.options(**opts):
        dev.depth(s, d, bits_in, bits_out, dither, full)
    return [dev.download(x) for x in d]


def check_sizes(dev, sizes, bits_in, bits_out, dither, full=False, **opts):
    outs = run(dev, [plane(i, h, w, bits_in) for i, (h, w) in enumerate(sizes)], bits_in, bits_out, dither, full, **opts)
    for i, ((h, w), o) in enumerate(zip(sizes, outs)):
        e = want(i, h, w, bits_in, bits_out, dither, full)
        assert o.dtype == e.dtype and np.array_equal(o, e), (h, w, bits_in, bits_out, dither, full, opts, int((o != e).sum()), np.argwhere(o != e)[:4].tolist())


@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("bits_in,bits_out", DIFFUSE)
def test_error_diffusion(dev, bits_in, bits_out, full):
    check_sizes(dev, SIZES, bits_in, bits_out, dr.ERROR_DIFFUSION, full)


@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("bits_in,bits_out", NONE)
def test_none(dev, bits_in, bits_out, full):
    check_sizes(dev, SIZES + [(5, 1000), (3, 4099)], bits_in, bits_out, dr.NONE, full)


@pytest.mark.parametrize("waves", [4, 16])
def test_either_workgroup_on_every_size(dev, waves):
    """VSZIP_DEPTH_WAVES forces one workgroup size on planes the row rule would give the other"""
    assert dev.get_option("VSZIP_DEPTH_WAVES") == 0
    check_sizes(dev, SIZES, 16, 8, dr.ERROR_DIFFUSION, VSZIP_DEPTH_WAVES=waves)


@pytest.mark.parametrize("waves", [0, 4])
def test_more_rows_than_a_workgroup_holds(dev, waves):
    """1030 x 40: 17 bands on 16 waves, or on 4 (five sweeps); the seam between the last wave and the first is the carry row in LDS"""
    check_sizes(dev, [(1030, 40)], 16, 8, dr.ERROR_DIFFUSION, VSZIP_DEPTH_WAVES=waves)
    check_sizes(dev, [(1030, 40)], 16, 10, dr.ERROR_DIFFUSION, True, VSZIP_DEPTH_WAVES=waves)


def test_rows_so_wide_that_a_band_waits_for_its_wave(dev):
    """900 columns take 17 chunks a band, more than the 12 the four waves' lags add up to: a wave's next band starts when the wave is free"""
    check_sizes(dev, [(300, 900), (270, 1283)], 16, 8, dr.ERROR_DIFFUSION, VSZIP_DEPTH_WAVES=4)


def test_the_carry_row_leaves_lds_for_scratch(dev):
    """4100 columns: beyond the 4096 of the LDS carry row. With five rows no carry is needed (one band); 260 rows under the small workgroup are
    five bands on four waves, whose fifth reads the carry row from the context's scratch. 4096 columns: the widest row that stays in LDS."""
    check_sizes(dev, [(5, 4100)], 16, 8, dr.ERROR_DIFFUSION)
    check_sizes(dev, [(260, 4100), (258, 4096), (3, 5000)], 16, 8, dr.ERROR_DIFFUSION, VSZIP_DEPTH_WAVES=4)


@pytest.mark.parametrize("bits_in,bits_out,dither", [(16, 8, 1), (10, 8, 1), (16, 10, 1), (8, 16, 0), (16, 8, 0)])
def test_unaligned_bases_and_odd_pitches_give_the_same_bits(dev, bits_in, bits_out, dither):
    """every pointer one to three samples off a 16-byte boundary and every pitch odd, each in turn and both together"""
    h, w = 70, 203
    src, e = plane(3, h, w, bits_in), want(3, h, w, bits_in, bits_out, dither, False)
    keep = []

    def shifted(a, shift, pitch):
        big = dev.empty(a.shape[0] + 1, pitch + 32, a.dtype)
        keep.append(big)
        v = dev.wrap(big.ptr + shift * a.itemsize, a.shape[0], a.shape[1], pitch, a.dtype)
        dev.copy_in(v, np.ascontiguousarray(a))
        dev.sync()
        return v
    for which in ("src", "dst", "all"):
        for shift in (1, 2, 3):
            on = lambda k: which in (k, "all")
            s = shifted(src, shift if on("src") else 0, 211 if on("src") else 224)
            d = shifted(np.zeros((h, w), dr.dtype_of(bits_out)), shift if on("dst") else 0, 213 if on("dst") else 224)
            dev.depth([s], [d], bits_in, bits_out, dither)
            assert np.array_equal(dev.download(d), e), (which, shift)


def test_200_planes_of_mixed_sizes_in_one_call(dev):
    sizes = [(1 + (i * 7) % 71, 1 + (i * 13) % 97) for i in range(197)] + [(257, 33), (300, 5), (64, 300)]
    check_sizes(dev, sizes, 16, 8, dr.ERROR_DIFFUSION)
    check_sizes(dev, sizes, 8, 16, dr.NONE)


def test_natural_content(dev):
    a = fx.tiled_natural((140, 333), np.uint16)
    n = fx.splitmix64_plane(3, (140, 333), np.uint16) >> 8
    for src in (a, (a // 2 + n).astype(np.uint16)):
        for bits_out, full in ((8, False), (10, False), (8, True)):
            got = run(dev, [src], 16, bits_out, dr.ERROR_DIFFUSION, full)[0]
            assert np.array_equal(got, dr.convert(src, 16, bits_out, dr.ERROR_DIFFUSION, full)), (bits_out, full)
    a8 = fx.tiled_natural((140, 333), np.uint8)
    assert np.array_equal(run(dev, [a8], 8, 16, dr.NONE)[0], a8.astype(np.uint16) << 8)
    assert np.array_equal(run(dev, [a8], 8, 16, dr.NONE, True)[0], a8.astype(np.uint16) * np.uint16(257))


def test_the_same_call_twice_gives_the_same_bytes(dev):
    sizes = [(129, 129), (1030, 40), (65, 300)]
    srcs = [dev.upload(plane(i, h, w, 16)) for i, (h, w) in enumerate(sizes)]
    dsts = [dev.empty(h, w, np.uint8) for h, w in sizes]
    call = dev.prepared_depth(srcs, dsts, 16, 8, dr.ERROR_DIFFUSION)
    call()
    first = [dev.download(d) for d in dsts]
    call()
    for (h, w), d, a, i in zip(sizes, dsts, first, range(3)):
        assert np.array_equal(dev.download(d), a) and np.array_equal(a, want(i, h, w, 16, 8, 1, False)), (h, w)


def test_argument_errors(dev):
    s16, d8, d16 = dev.upload(np.zeros((8, 8), np.uint16)), dev.empty(8, 8, np.uint8), dev.empty(8, 8, np.uint16)
    for args, kw, code, msg in [((17, 8), {}, -1, "Depth: bits_in 17 is outside 8..16"), ((16, 7), {}, -1, "Depth: bits_out 7 is outside 8..16"),
                                ((16, 8, 2), {}, -1, r"Depth: dither 2 is neither 0 \(none\) nor 1 \(error diffusion\)"),
                                ((16, 8, 1), dict(full_range=True, chroma=True), -3, r"Depth: plane 0: full-range chroma is not built \(DESIGN.md section 1\)")]:
        with pytest.raises(VszipError, match=msg) as e:
            dev.depth([s16], [d8], *args, **kw)
        assert e.value.code == code
    short = dev.wrap(d8.ptr, 8, 8, 4, np.uint8)
    with pytest.raises(VszipError, match="Depth: plane 0: bad geometry 8x8, pitches 32 -> 4"):
        dev.depth([s16], [short], 16, 8, 1)
    with pytest.raises(ValueError, match="8-bit destination planes are uint8"):
        dev.depth([s16], [d16], 16, 8)
    dev.depth([s16], [d8], 16, 8, 1, chroma=True)  # limited-range chroma is served
    assert not dev.download(d8).any()
