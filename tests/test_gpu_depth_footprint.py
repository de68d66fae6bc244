"""GPU footprint of vszip_depth: the "Plane memory" clauses of include/vszip_hip.h (readable extent, independence, written extent) through the
guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py uses, for both dithers and both directions: guards, pitch
padding, a window's live neighbours and every source come back as uploaded; only `[0, w) x h` of each destination is written and it equals the
spec (tests/depth_ref.py) bit for bit; the runs with poison 0x00 and 0xFF around the planes give the same bits."""
import numpy as np
import pytest

import depth_ref as dr
from test_gpu_footprint import LAYOUTS, Case, sizes_for

pytestmark = pytest.mark.gpu

CONVERSIONS = [(16, 8, dr.ERROR_DIFFUSION), (16, 10, dr.ERROR_DIFFUSION), (10, 8, dr.ERROR_DIFFUSION), (8, 8, dr.ERROR_DIFFUSION), (8, 16, dr.NONE), (16, 8, dr.NONE),
               (12, 16, dr.NONE)]
IDS = [f"{a}-{b}-{'diffuse' if d else 'none'}" for a, b, d in CONVERSIONS]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _run(dev, layout, sizes, bits_in, bits_out, dither, seed, full=False):
    c = Case(layout, seed)
    srcs = []
    for i, (h, w) in enumerate(sizes):
        a = dr.content(seed + i, h, w, bits_in)
        srcs.append(a)
        c.add(f"src{i}", "in", a.dtype, h, w, a)
        c.add(f"dst{i}", "out", dr.dtype_of(bits_out), h, w)
    n = len(srcs)

    def call(P):
        dev.depth([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], bits_in, bits_out, dither, full)
    c.run(dev, call, {f"dst{i}": dr.convert(a, bits_in, bits_out, dither, full) for i, a in enumerate(srcs)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits_in,bits_out,dither", CONVERSIONS, ids=IDS)
def test_depth(dev, bits_in, bits_out, dither, layout):
    _run(dev, layout, sizes_for(layout, 70, 83, 3, 1, 1), bits_in, bits_out, dither, 4)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits_in,bits_out,dither", CONVERSIONS[:2] + CONVERSIONS[4:6], ids=IDS[:2] + IDS[4:6])
def test_small_planes_and_whole_groups(dev, bits_in, bits_out, dither, layout):
    _run(dev, layout, [(1, 1), (7, 13), (2, 16), (3, 64), (5, 17), (66, 8)] if layout == "packed" else [(3, 5), (2, 64), (1, 16)], bits_in, bits_out, dither, 7, full=True)


@pytest.mark.parametrize("layout", ["tight_odd", "window"])
def test_more_rows_than_the_small_workgroup_holds(dev, layout):
    """five bands on four waves: the carry row is in use while the footprint is watched"""
    with dev.options(VSZIP_DEPTH_WAVES=4):
        _run(dev, layout, [(260, 37)], 16, 8, dr.ERROR_DIFFUSION, 9)
