"""GPU footprint of vszip_color_map: the "Plane memory" clauses of include/vszip_hip.h (readable extent, independence, written extent)
through the guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py uses: guards, pitch padding, a window's live
neighbours and every source come back as uploaded; only `[0, w) x h` of each of the three outputs is written and it equals the spec
(tests/color_map_ref.py) bit for bit; the runs with poison 0x00 and 0xFF around the planes give the same bits."""
import numpy as np
import pytest

import color_map_ref as cm
from test_gpu_footprint import LAYOUTS, Case, sizes_for

pytestmark = pytest.mark.gpu

LUT = cm.permutation_lut(1)


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _run(dev, layout, sizes, seed):
    c = Case(layout, seed)
    planes = []
    for i, (h, w) in enumerate(sizes):
        p = cm.gpu_plane(seed + i, w, h)
        planes.append(p)
        c.add(f"src{i}", "in", np.uint8, h, w, p)
        for name in "rgb":
            c.add(f"{name}{i}", "out", np.uint8, h, w)
    n = len(planes)

    def call(P):
        pick = lambda name: [P[f"{name}{i}"] for i in range(n)]
        dev.color_map(pick("src"), pick("r"), pick("g"), pick("b"), LUT)
    expect = {}
    for i, p in enumerate(planes):
        for name, e in zip("rgb", cm.apply(p, LUT)):
            expect[f"{name}{i}"] = e
    c.run(dev, call, expect)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", [3, 4, 5], ids=["natural", "noise", "every-value"])
def test_color_map(dev, seed, layout):
    _run(dev, layout, sizes_for(layout, 37, 83, 3, 1, 1), seed)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_small_frames_and_whole_groups(dev, layout):
    _run(dev, layout, [(1, 1), (7, 13), (2, 16), (3, 64), (5, 17)] if layout == "packed" else [(3, 5), (2, 64), (1, 16)], 7)
