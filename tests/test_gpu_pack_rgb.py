"""GPU: vszip_pack_rgb against the numpy spec (tests/pack_rgb_ref.py), bit for bit: widths around every step of the kernel's mappings
(a lane's group of samples, a wave, the workgroup's 256 lanes, one sweep of the workgroup) and heights around its rows per workgroup, in
one call and each alone; natural content and noise; RGB30 samples above 1023; 200 frames in one call; unaligned bases and odd
pitches; r, g and b as one pointer; the reference's golden inputs through the device; and the argument errors."""
import numpy as np
import pytest

import pack_rgb_ref as pr
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu

# 4101: beyond what the 256 lanes of a workgroup cover in one sweep at 16 samples a lane (4096), so at 4 a lane (1024), too
WIDTHS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4101]
HEIGHTS = [1, 2, 3, 7, 37]
SIZES = [(h, w) for w in WIDTHS for h in HEIGHTS]
DT = {8: np.uint8, 10: np.uint16}


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def check(dev, frames, bits):
    """frames: (r, g, b) host planes"""
    ups = [[dev.upload(p) for p in f] for f in frames]
    dsts = [dev.empty(f[0].shape[0], f[0].shape[1], np.uint32) for f in frames]
    dev.pack_rgb([u[0] for u in ups], [u[1] for u in ups], [u[2] for u in ups], dsts, bits)
    for i, (f, d) in enumerate(zip(frames, dsts)):
        o, e = dev.download(d), pr.pack(*f, bits)
        assert o.dtype == e.dtype and o.shape == e.shape and np.array_equal(o, e), (i, e.shape, bits, int((o != e).sum()))


@pytest.mark.parametrize("content", [0, 1], ids=["natural", "noise"])
@pytest.mark.parametrize("bits", [8, 10])
def test_every_size_in_one_call(dev, bits, content):
    """80 frames; the ones of several workgroups (37 rows, 4101 columns) stand between small ones"""
    order = np.random.default_rng(3).permutation(len(SIZES))
    frames = [pr.gpu_frame(2 * int(k) + content, SIZES[k][1], SIZES[k][0], bits) for k in order]
    if bits == 10 and content == 1:
        assert max(int(p.max()) for f in frames for p in f) == 65535  # samples above 1023, the largest included
    check(dev, frames, bits)


@pytest.mark.parametrize("bits", [8, 10])
def test_every_size_alone(dev, bits):
    for k, (h, w) in enumerate(SIZES):
        check(dev, [pr.gpu_frame(k, w, h, bits)], bits)


def test_rgb30_samples_above_1023_wrap_as_the_reference_does(dev):
    r, g, b = (np.ascontiguousarray(p) for p in pr.gpu_frame(1, 67, 5, 10))
    r[0, :4], g[0, :4], b[0, :4] = (65535, 0, 0, 65535), (0, 65535, 0, 65535), (0, 0, 65535, 65535)
    r[1, 0], g[1, 0], b[1, 0] = 1024, 1, 2047
    check(dev, [(r, g, b)], 10)
    s, d = dev.upload(r), dev.empty(5, 67, np.uint32)
    z = dev.upload(np.zeros_like(r))
    dev.pack_rgb([s], [z], [z], [d], 10)
    assert int(dev.download(d)[0, 0]) == 0xFFF00000


@pytest.mark.parametrize("bits", [8, 10])
def test_200_frames_in_one_call(dev, bits):
    """more than one launch, whatever the table holds (at most 192)"""
    frames = [pr.gpu_frame(i, 1 + (i * 7) % 41, 1 + i % 9, bits) for i in range(200)]
    check(dev, frames, bits)


@pytest.mark.parametrize("bits", [8, 10])
def test_unaligned_bases_and_odd_pitches_give_the_same_bits(dev, bits):
    """base offsets of 1 .. 15 bytes (whole samples) and odd pitches, on one input, on the output and on all planes; and 16-byte aligned with a
    large pitch"""
    keep = []

    def shifted(a, shift, pitch):
        isz = a.dtype.itemsize
        big = dev.empty(a.shape[0] + 1, pitch + 32, a.dtype)
        keep.append(big)
        v = dev.wrap(big.ptr + shift, a.shape[0], a.shape[1], pitch, a.dtype)
        assert shift % isz == 0
        dev.copy_in(v, np.ascontiguousarray(a))
        return v

    isz = 1 if bits == 8 else 2
    for seed, (h, w) in ((4, (7, 83)), (5, (5, 130))):
        f = pr.gpu_frame(seed, w, h, bits)
        want, zeros = pr.pack(*f, bits), np.zeros((h, w), np.uint32)
        for shift in range(1, 16):
            for which in ("r", "g", "b", "dst", "all"):
                ins = []
                for name, p in zip("rgb", f):
                    on = which in (name, "all") and shift % isz == 0
                    ins.append(shifted(p, shift if on else 0, w + 1 + 2 * shift if which in (name, "all") else 160))
                on = which in ("dst", "all") and shift % 4 == 0
                d = shifted(zeros, shift if on else 0, w + 3 + 2 * shift if which in ("dst", "all") else 160)
                dev.pack_rgb([ins[0]], [ins[1]], [ins[2]], [d], bits)
                assert np.array_equal(dev.download(d), want), (bits, (h, w), shift, which)
        ins = [shifted(p, 16 * (k + 1), 1024) for k, p in enumerate(f)]
        d = shifted(zeros, 48, 2048)
        dev.pack_rgb([ins[0]], [ins[1]], [ins[2]], [d], bits)
        assert np.array_equal(dev.download(d), want)
    dev.sync()


@pytest.mark.parametrize("bits", [8, 10])
def test_r_g_and_b_as_one_pointer(dev, bits):
    p = pr.gpu_frame(1, 130, 7, bits)[0]
    s, d = dev.upload(p), dev.empty(7, 130, np.uint32)
    dev.pack_rgb([s], [s], [s], [d], bits)
    assert np.array_equal(dev.download(d), pr.pack(p, p, p, bits))
    assert np.array_equal(dev.download(s), p)


@pytest.mark.parametrize("key", sorted(pr.goldens()))
def test_golden_inputs_through_the_device_give_the_golden_stats(dev, key):
    fmt, geom, _ = key.split("|")
    r, g, b, bits = pr.golden_inputs(fmt, geom)
    d = dev.empty(r.shape[0], r.shape[1], np.uint32)
    dev.pack_rgb([dev.upload(r)], [dev.upload(g)], [dev.upload(b)], [d], bits)
    o = dev.download(d)
    assert np.array_equal(o, pr.pack(r, g, b, bits))
    st, want = pr.stats(o), pr.goldens()[key]["p0"]
    assert st["min"] == want["min"] and st["max"] == want["max"] and st["avg"] == pytest.approx(want["avg"], rel=1e-12, abs=0), (key, st, want)


def test_argument_errors(dev):
    p8, p16 = np.zeros((20, 20), np.uint8), np.zeros((20, 20), np.uint16)
    s8, s16, d = dev.upload(p8), dev.upload(p16), dev.empty(20, 20, np.uint32)
    dev.copy_in(d, np.full((20, 20), 7, np.uint32))
    for bits in (0, 9, 12, 16, -8):
        with pytest.raises(VszipError, match="PackRGB: only RGB24 and RGB30 inputs are supported!") as ei:
            dev.pack_rgb([s16], [s16], [s16], [d], bits)
        assert ei.value.code == -1
    null8 = dev.wrap(0, 20, 20, 32, np.uint8)
    for k in range(4):
        planes = [[s8, null8][k == j] for j in range(3)] + [dev.wrap(0, 20, 20, 32, np.uint32) if k == 3 else d]
        with pytest.raises(VszipError, match="PackRGB: frame 1: r, g, b and dst must not be NULL") as ei:
            dev.pack_rgb([s8, planes[0]], [s8, planes[1]], [s8, planes[2]], [d, planes[3]], 8)
        assert ei.value.code == -1
    short8, shortd = dev.wrap(s8.ptr, 20, 20, 19, np.uint8), dev.wrap(d.ptr, 20, 20, 19, np.uint32)
    for k in range(4):
        planes = [[s8, short8][k == j] for j in range(3)] + [shortd if k == 3 else d]
        with pytest.raises(VszipError, match=r"PackRGB: frame 0: bad geometry 20x20, pitches \d+ / \d+ / \d+ -> \d+") as ei:
            dev.pack_rgb([planes[0]], [planes[1]], [planes[2]], [planes[3]], 8)
        assert ei.value.code == -1
    for h, w in ((0, 20), (20, 0), (-1, 20)):
        with pytest.raises(VszipError, match=r"PackRGB: frame 0: bad geometry") as ei:
            dev.pack_rgb([s8], [s8], [s8], [dev.wrap(d.ptr, h, w, 32, np.uint32)], 8)  # (the binding takes a frame's size from its dst)
        assert ei.value.code == -1
    with pytest.raises(ValueError, match="bits=8 takes uint8 planes"):
        dev.pack_rgb([s16], [s16], [s16], [d], 8)
    with pytest.raises(ValueError, match="bits=10 takes uint16 planes"):
        dev.pack_rgb([s8], [s8], [s8], [d], 10)
    with pytest.raises(ValueError, match="dst planes are uint32"):
        dev.pack_rgb([s8], [s8], [s8], [s8], 8)
    assert np.array_equal(dev.download(d), np.full((20, 20), 7, np.uint32))  # nothing was written by the refused calls
    dev.pack_rgb([s8], [s8], [s8], [d], 8)  # and the valid call goes through: black, opaque
    assert np.array_equal(dev.download(d), np.full((20, 20), 0xFF000000, np.uint32))
