"""The BoxBlur ring kernel's row queue (16-bit planes: rows requested several steps ahead straight into LDS, one hand-counted wait a step,
boxblur_ct.hpp RingGeom::QD) against the CPU oracle, bit for bit, at the smallest shapes where the queue can go wrong: one-period bands at both
plane edges, interior bands whose requests stop beside live rows, bands of several periods (the queue slot wraps across ring periods), the radii at
the ends of the K ring's sizes, a plane with a general strip, and a padded source pitch. A miscounted wait shows as rare wrong rows, so every case
launches 20 times and wants 20 identical outputs. Contents: full-range noise, and all-65535 planes (the sums at their largest)."""
import numpy as np
import pytest

import fixtures as fx

pytestmark = pytest.mark.gpu

RUNS = 20


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _plane(content, seed, shape, dtype):
    if content == "noise":
        return fx.splitmix64_plane(0x9F370000 + seed, shape, dtype)
    return np.full(shape, np.iinfo(dtype).max, dtype)


def _run_and_check(dev, srcs, dsts, want_of, r):
    """RUNS launches over one plane table; plane i of the first run equals want_of[i], every later run equals the first."""
    table = dev.plane_table(srcs, dsts)
    first = None
    for run in range(RUNS):
        dev.boxblur_table(dsts[0].dtype, table, r, 1, r, 1)
        got = [dev.download(d) for d in dsts]
        if first is None:
            for i, (g, w) in enumerate(zip(got, want_of)):
                bad = g != w
                assert not bad.any(), (i, g.shape, r, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            first = got
        else:
            for i, (g, f) in enumerate(zip(got, first)):
                assert np.array_equal(g, f), (run, i, np.argwhere(g != f)[:4].tolist())


def _check_planes(dev, oracle, planes, r):
    srcs = [dev.upload(p) for p in planes]
    dsts = [dev.empty(p.shape[0], p.shape[1], p.dtype) for p in planes]
    _run_and_check(dev, srcs, dsts, [oracle.boxblur(p, r, 1, r, 1) for p in planes], r)


CONTENTS = ["noise", "max"]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("h", [56, 53, 57])
def test_one_period_bands_at_both_edges(dev, oracle, content, h):
    """r = 13 (ring period 28): 480 x 56 is two one-period bands that each touch a plane edge; 53 and 57 rows shift the last band up over its neighbour."""
    _check_planes(dev, oracle, [_plane(content, h, (h, 480), np.uint16)], 13)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("h", [140, 141])
def test_interior_bands(dev, oracle, content, h):
    """Five (six) one-period bands a plane: the interior ones take the plain path and stop requesting rows beside rows their neighbours need;
    960 x 140 goes with its 480 x 70 chroma planes in one call."""
    planes = [_plane(content, 10 + h, (h, 960), np.uint16)]
    if h == 140:
        planes += [_plane(content, 20 + k, (70, 480), np.uint16) for k in range(2)]
    _check_planes(dev, oracle, planes, 13)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("h", [1120, 1121])
def test_bands_of_several_periods(dev, oracle, content, h):
    """192 planes of 480 x 1120 are planned as 10 bands of 4 periods each, 192 of 480 x 1121 as 14 bands of about 3 periods with the last one shifted
    (ring_plan: small inputs get one-period bands only). Three distinct source planes, 192 destinations, every one compared."""
    base = [_plane(content, 30 + k, (h, 480), np.uint16) for k in range(3)]
    want = [oracle.boxblur(p, 13, 1, 13, 1) for p in base]
    up = [dev.upload(p) for p in base]
    srcs = [up[k % 3] for k in range(192)]
    dsts = [dev.empty(h, 480, np.uint16) for _ in range(192)]
    _run_and_check(dev, srcs, dsts, [want[k % 3] for k in range(192)], 13)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("r", [1, 2, 19, 22])
def test_radii_at_the_ends(dev, oracle, content, r):
    """The smallest window, the ring sizes on either side of the register tiers, and the largest K ring (r = 22: three lanes of K columns, 46 + QD entries)."""
    _check_planes(dev, oracle, [_plane(content, 40 + r, (140, 960), np.uint16)], r)


@pytest.mark.parametrize("content", CONTENTS)
def test_width_with_a_general_strip(dev, oracle, content):
    """488 columns: one fast tile (queued rows) and a general strip in a second launch."""
    _check_planes(dev, oracle, [_plane(content, 50, (140, 488), np.uint16)], 13)


@pytest.mark.parametrize("content", CONTENTS)
def test_source_pitch_larger_than_width(dev, oracle, content):
    """A 960-column plane inside rows of 1024 samples whose padding holds 0x5A5A: the requests take the pitch from the table and nothing of the padding
    reaches the output."""
    h, w, pitch = 140, 960, 1024
    p = _plane(content, 60, (h, w), np.uint16)
    wide = np.full((h, pitch), 0x5A5A, np.uint16)
    wide[:, :w] = p
    up = dev.upload(wide)
    assert up.stride == pitch
    src = dev.wrap(up.ptr, h, w, up.stride, np.uint16)
    dst = dev.empty(h, w, np.uint16)
    _run_and_check(dev, [src], [dst], [oracle.boxblur(p, 13, 1, 13, 1)], 13)
