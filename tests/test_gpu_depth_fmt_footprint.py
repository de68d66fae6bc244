"""GPU footprint of vszip_depth_fmt: the "Plane memory" clauses of include/vszip_hip.h through the guarded arena (tests/guarded.py), over the six
layouts tests/test_gpu_footprint.py uses, for u8 -> f32, f32 -> u8 none, f32 -> u8 error diffusion and f32 -> f16: guards, pitch padding, a
window's live neighbours and every source come back as uploaded; only `[0, w) x h` of each destination is written and it equals the spec
(tests/depth_fmt_ref.py) bit for bit; the runs with poison 0x00 and 0xFF around the planes give the same bits."""
import pytest

import depth_fmt_ref as df
import depth_ref as dr
from test_gpu_footprint import LAYOUTS, Case, sizes_for

pytestmark = pytest.mark.gpu

U8, F16, F32 = (df.U8, 8), (df.F16, 16), (df.F32, 32)
CONVERSIONS = [(U8, F32, df.NONE), (F32, U8, df.NONE), (F32, U8, df.ERROR_DIFFUSION), (F32, F16, df.NONE)]
IDS = ["u8-f32", "f32-u8-none", "f32-u8-diffuse", "f32-f16"]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _run(dev, layout, sizes, tin, tout, dither, seed):
    c = Case(layout, seed)
    srcs = []
    for i, (h, w) in enumerate(sizes):
        a = df.content(seed + i, h, w, 8, True) if df.is_float(tin[0]) else dr.content(seed + i, h, w, 8)
        srcs.append(a)
        c.add(f"src{i}", "in", a.dtype, h, w, a)
        c.add(f"dst{i}", "out", df.NP[tout[0]], h, w)
    n = len(srcs)

    def call(P):
        dev.depth_fmt([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], *tin, *tout, dither, True)
    c.run(dev, call, {f"dst{i}": df.convert(a, *tin, *tout, dither, True) for i, a in enumerate(srcs)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tin,tout,dither", CONVERSIONS, ids=IDS)
def test_depth_fmt(dev, tin, tout, dither, layout):
    _run(dev, layout, sizes_for(layout, 70, 83, 3, 1, 1), tin, tout, dither, 4)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tin,tout,dither", CONVERSIONS, ids=IDS)
def test_small_planes_and_whole_groups(dev, tin, tout, dither, layout):
    _run(dev, layout, [(1, 1), (7, 13), (2, 16), (3, 64), (5, 17), (66, 8)] if layout == "packed" else [(3, 5), (2, 64), (1, 16)], tin, tout, dither, 7)


@pytest.mark.parametrize("layout", ["tight_odd", "window"])
def test_more_rows_than_the_small_workgroup_holds(dev, layout):
    """five bands on four waves: the carry row is in use while the footprint is watched"""
    with dev.options(VSZIP_DEPTH_WAVES=4):
        _run(dev, layout, [(260, 37)], F32, U8, df.ERROR_DIFFUSION, 9)
