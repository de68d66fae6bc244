"""GPU: vszip_color_map against the numpy spec (tests/color_map_ref.py), bit for bit, through a table of three distinct random
permutations (a swapped channel or an index off by one cannot pass): widths around every step of the kernel's mapping (a lane's 16
samples, a wave, the workgroup's 256 lanes, one sweep of the workgroup) and heights around its rows per workgroup, in one call and each
alone; natural content, noise and planes that hold every value; 200 frames in one call; unaligned bases and odd pitches; the table
overwritten right after the call; the reference's golden inputs through the device; and the argument errors."""
import numpy as np
import pytest

import color_map_ref as cm
import fixtures as fx
from vszip_amd import capi
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu

# 4101: beyond what the 256 lanes of a workgroup cover in one sweep at 16 samples a lane (4096)
WIDTHS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4101]
HEIGHTS = [1, 2, 3, 7, 37]
SIZES = [(h, w) for w in WIDTHS for h in HEIGHTS]
LUT = cm.permutation_lut(0)


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def check(dev, planes, table=LUT):
    srcs = [dev.upload(p) for p in planes]
    outs = [[dev.empty(p.shape[0], p.shape[1], np.uint8) for p in planes] for _ in range(3)]
    dev.color_map(srcs, outs[0], outs[1], outs[2], table)
    for i, p in enumerate(planes):
        for c, e in enumerate(cm.apply(p, table)):
            o = dev.download(outs[c][i])
            assert o.dtype == e.dtype and o.shape == e.shape and np.array_equal(o, e), (i, p.shape, "rgb"[c], int((o != e).sum()))


@pytest.mark.parametrize("content", [0, 1, 2], ids=["natural", "noise", "every-value"])
def test_every_size_in_one_call(dev, content):
    """80 frames; the ones of several workgroups (37 rows, 4101 columns) stand between small ones"""
    order = np.random.default_rng(3).permutation(len(SIZES))
    planes = [cm.gpu_plane(3 * int(k) + content, SIZES[k][1], SIZES[k][0]) for k in order]
    if content == 2:
        assert sum(len(np.unique(p)) == 256 for p in planes) >= 25  # every plane of 256 columns or more
    check(dev, planes)


def test_every_size_alone(dev):
    for k, (h, w) in enumerate(SIZES):
        check(dev, [cm.gpu_plane(k, w, h)])


def test_every_value_through_an_analytic_table(dev):
    table = capi.color_map_lut(*cm.analytic_palette("winter"))
    p = np.arange(256, dtype=np.uint8).reshape(1, 256)
    check(dev, [p, np.ascontiguousarray(p[:, ::-1]), cm.gpu_plane(2, 300, 9)], table)


def test_200_frames_in_one_call(dev):
    """more than one launch, whatever the table holds (at most 192)"""
    check(dev, [cm.gpu_plane(i, 1 + (i * 7) % 41, 1 + i % 9) for i in range(200)])


def test_unaligned_bases_and_odd_pitches_give_the_same_bits(dev):
    """base offsets of 1 .. 15 bytes and odd pitches, on the source, on each output and on all planes; and 16-byte aligned with a large pitch"""
    keep = []

    def shifted(a, shift, pitch):
        big = dev.empty(a.shape[0] + 1, pitch + 32, np.uint8)
        keep.append(big)
        v = dev.wrap(big.ptr + shift, a.shape[0], a.shape[1], pitch, np.uint8)
        dev.copy_in(v, np.ascontiguousarray(a))
        return v

    for seed, (h, w) in ((3, (7, 83)), (4, (5, 130)), (5, (3, 67))):
        p = cm.gpu_plane(seed, w, h)
        want, zeros = cm.apply(p, LUT), np.zeros_like(p)
        for shift in range(1, 16):
            for which in ("src", "r", "g", "b", "all"):
                on = lambda name: which in (name, "all")
                s = shifted(p, shift if on("src") else 0, w + 1 + 2 * shift if on("src") else 160)
                outs = [shifted(zeros, shift if on(n) else 0, w + 3 + 2 * shift + k if on(n) else 160) for k, n in enumerate("rgb")]
                dev.color_map([s], [outs[0]], [outs[1]], [outs[2]], LUT)
                for c in range(3):
                    assert np.array_equal(dev.download(outs[c]), want[c]), ((h, w), shift, which, "rgb"[c])
        s = shifted(p, 16, 1024)
        outs = [shifted(zeros, 16 * (k + 2), 2048) for k in range(3)]
        dev.color_map([s], [outs[0]], [outs[1]], [outs[2]], LUT)
        for c in range(3):
            assert np.array_equal(dev.download(outs[c]), want[c])
    dev.sync()


def test_the_table_is_consumed_before_the_call_returns(dev):
    p = cm.gpu_plane(1, 1025, 37)
    s = dev.upload(p)
    outs = [dev.empty(37, 1025, np.uint8) for _ in range(3)]
    table = LUT.copy()
    dev.color_map([s], [outs[0]], [outs[1]], [outs[2]], table)
    table[:] = 0  # overwritten at once, before the stream is drained
    for c, e in enumerate(cm.apply(p, LUT)):
        assert np.array_equal(dev.download(outs[c]), e)


@pytest.mark.parametrize("key", sorted(cm.goldens()))
def test_golden_inputs_through_the_device_give_the_golden_stats(dev, key):
    y, color = cm.golden_input(key)
    table = capi.color_map_lut(*cm.palette_of_color(color))
    outs = [dev.empty(y.shape[0], y.shape[1], np.uint8) for _ in range(3)]
    dev.color_map([dev.upload(y)], [outs[0]], [outs[1]], [outs[2]], table)
    for i, e in enumerate(cm.apply(y, cm.lut(*cm.palette_of_color(color)))):
        o = dev.download(outs[i])
        assert np.array_equal(o, e)
        st, g = fx.plane_stats(o), cm.goldens()[key][f"p{i}"]
        assert st["min"] == g["min"] and st["max"] == g["max"] and st["avg"] == pytest.approx(g["avg"], rel=1e-12, abs=0), (key, i, st, g)


def test_argument_errors(dev):
    src = dev.upload(np.full((20, 20), 9, np.uint8))
    outs = [dev.empty(20, 20, np.uint8) for _ in range(3)]
    for o in outs:
        dev.copy_in(o, np.full((20, 20), 7, np.uint8))
    with pytest.raises(VszipError, match="ColorMap: lut must not be NULL") as ei:
        dev.color_map([src], [outs[0]], [outs[1]], [outs[2]], None)
    assert ei.value.code == -1
    null = dev.wrap(0, 20, 20, 32, np.uint8)
    for k in range(4):
        pl = [null if k == j else q for j, q in enumerate([src] + outs)]
        with pytest.raises(VszipError, match="ColorMap: frame 1: src, r, g and b must not be NULL") as ei:
            dev.color_map([src, pl[0]], [outs[0], pl[1]], [outs[1], pl[2]], [outs[2], pl[3]], LUT)
        assert ei.value.code == -1
    for k in range(4):
        pl = [dev.wrap(q.ptr, 20, 20, 19, np.uint8) if k == j else q for j, q in enumerate([src] + outs)]
        with pytest.raises(VszipError, match=r"ColorMap: frame 0: bad geometry 20x20, pitches \d+ -> \d+ / \d+ / \d+") as ei:
            dev.color_map([pl[0]], [pl[1]], [pl[2]], [pl[3]], LUT)
        assert ei.value.code == -1
    for h, w in ((0, 20), (20, 0), (20, -3)):
        with pytest.raises(VszipError, match="ColorMap: frame 0: bad geometry") as ei:
            dev.color_map([dev.wrap(src.ptr, h, w, 32, np.uint8)], [outs[0]], [outs[1]], [outs[2]], LUT)
        assert ei.value.code == -1
    with pytest.raises(ValueError, match="8-bit planes only"):
        dev.color_map([dev.upload(np.zeros((8, 8), np.uint16))], [outs[0]], [outs[1]], [outs[2]], LUT)
    with pytest.raises(ValueError, match=r"\(3, 256\) uint8"):
        dev.color_map([src], [outs[0]], [outs[1]], [outs[2]], LUT.astype(np.int32))
    for o in outs:
        assert np.array_equal(dev.download(o), np.full((20, 20), 7, np.uint8))  # nothing was written by the refused calls
    dev.color_map([src], [outs[0]], [outs[1]], [outs[2]], LUT)  # and the valid call goes through
    for c in range(3):
        assert np.array_equal(dev.download(outs[c]), np.full((20, 20), LUT[c][9], np.uint8))
