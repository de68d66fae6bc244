"""The BoxBlur ring kernel's row bands (boxblur_ct.hpp, ring_bands.hpp) against the CPU oracle, bit for bit: a band is any number of rows from one ring
period up, no band is shifted over its neighbour, and the row loop leaves a ring period behind the band's last row. The shapes are the smallest at which
that can go wrong: bands that end in the first, a middle and the last slot of a period, odd and even row counts (the last row is emitted from either
half of the prefix double buffer), a single band that ends inside a period, one-period bands beside longer ones, interior bands on the plain path, and
every form of the kernel (16- and 8-bit, 8 and 16 pixels a lane, queued and register-only rows, general strip, horizontal only). Every case runs
twice: the first run equals the oracle, the second equals the first. Contents: full-range noise, and all-max planes (the sums at their largest)."""
import numpy as np
import pytest

import fixtures as fx

pytestmark = pytest.mark.gpu

RUNS = 2
CONTENTS = ["noise", "max"]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _plane(content, seed, shape, dtype):
    if content == "noise":
        return fx.splitmix64_plane(0xBA2D0000 + seed, shape, dtype)
    return np.full(shape, np.iinfo(dtype).max, dtype)


def _run_and_check(dev, srcs, dsts, want_of, args):
    """RUNS launches over one plane table; plane i of the first run equals want_of[i], every later run equals the first."""
    table = dev.plane_table(srcs, dsts)
    first = None
    for run in range(RUNS):
        dev.boxblur_table(dsts[0].dtype, table, *args)
        got = [dev.download(d) for d in dsts]
        if first is None:
            for i, (g, w) in enumerate(zip(got, want_of)):
                bad = g != w
                assert not bad.any(), (i, g.shape, args, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            first = got
        else:
            for i, (g, f) in enumerate(zip(got, first)):
                assert np.array_equal(g, f), (run, i, np.argwhere(g != f)[:4].tolist())


def _check_planes(dev, oracle, planes, r, vr=None):
    args = (r, 1, r, 1) if vr is None else (r, 1, vr, 1 if vr else 0)  # (vradius = 0: vpasses = 0 too, the call that takes the ring kernel)
    srcs = [dev.upload(p) for p in planes]
    dsts = [dev.empty(p.shape[0], p.shape[1], p.dtype) for p in planes]
    _run_and_check(dev, srcs, dsts, [oracle.boxblur(p, *args) for p in planes], args)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("h", [56, 57, 83, 53])
def test_bands_that_end_inside_a_period(dev, oracle, content, h):
    """r = 13 (ring period 28), 480 columns. 56 rows: two one-period bands, each on a plane edge. 57 and 83: bands of 28 + 29 and 41 + 42 rows, which
    end in the last, the first and the middle slots of a period with odd and even row counts (both halves of the prefix double buffer). 53: a single
    band that ends inside its second period."""
    _check_planes(dev, oracle, [_plane(content, h, (h, 480), np.uint16)], 13)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("h", [140, 141])
def test_one_period_bands_and_interior_bands(dev, oracle, content, h):
    """960 x 140 with its two 480 x 70 chroma planes in one call, and 960 x 141: five bands a luma plane (an odd count; 141 rows: four of 28 and one
    of 29), the three interior ones on the plain path between a band on the top edge and one on the bottom edge; 35-row bands in the chroma planes."""
    planes = [_plane(content, 10 + h, (h, 960), np.uint16)]
    if h == 140:
        planes += [_plane(content, 20 + k, (70, 480), np.uint16) for k in range(2)]
    _check_planes(dev, oracle, planes, 13)


@pytest.mark.parametrize("content", CONTENTS)
def test_many_bands_of_several_periods(dev, oracle, content):
    """192 planes of 480 x 1121: many bands of several periods whose row counts differ by one (1121 is a prime), the queue slot and the K ring wrap
    across periods and stop wherever the band ends. Three distinct source planes, 192 destinations, every one compared."""
    h = 1121
    base = [_plane(content, 30 + k, (h, 480), np.uint16) for k in range(3)]
    want = [oracle.boxblur(p, 13, 1, 13, 1) for p in base]
    up = [dev.upload(p) for p in base]
    srcs = [up[k % 3] for k in range(192)]
    dsts = [dev.empty(h, 480, np.uint16) for _ in range(192)]
    _run_and_check(dev, srcs, dsts, [want[k % 3] for k in range(192)], (13, 1, 13, 1))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("r", [1, 2, 19, 22, 14])
def test_other_radii(dev, oracle, content, r):
    """960 x 141 at the smallest windows, the ring sizes on either side of the register tiers and the largest ring; r = 14 is the first radius whose
    rows stay in registers (no queue)."""
    _check_planes(dev, oracle, [_plane(content, 40 + r, (141, 960), np.uint16)], r)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("w", [960, 1920])
def test_8bit_planes(dev, oracle, content, w):
    """8-bit planes at r = 13, 141 rows: 960 columns take 8 pixels a lane, 1920 take 16."""
    _check_planes(dev, oracle, [_plane(content, 50 + w, (141, w), np.uint8)], 13)


@pytest.mark.parametrize("content", CONTENTS)
def test_width_with_a_general_strip(dev, oracle, content):
    """488 x 141: one fast tile and a general strip in a second launch, both banded by rows."""
    _check_planes(dev, oracle, [_plane(content, 60, (141, 488), np.uint16)], 13)


@pytest.mark.parametrize("content", CONTENTS)
def test_source_pitch_larger_than_width(dev, oracle, content):
    """A 960-column plane inside rows of 1024 samples whose padding holds 0x5A5A: nothing of the padding reaches the output."""
    h, w, pitch = 141, 960, 1024
    p = _plane(content, 70, (h, w), np.uint16)
    wide = np.full((h, pitch), 0x5A5A, np.uint16)
    wide[:, :w] = p
    up = dev.upload(wide)
    assert up.stride == pitch
    src = dev.wrap(up.ptr, h, w, up.stride, np.uint16)
    dst = dev.empty(h, w, np.uint16)
    _run_and_check(dev, [src], [dst], [oracle.boxblur(p, 13, 1, 13, 1)], (13, 1, 13, 1))


@pytest.mark.parametrize("content", CONTENTS)
def test_horizontal_only(dev, oracle, content):
    """vradius = 0 on 960 x 141: the one-row window's ring (period 2) under bands of any row count."""
    _check_planes(dev, oracle, [_plane(content, 80, (141, 960), np.uint16)], 13, vr=0)
