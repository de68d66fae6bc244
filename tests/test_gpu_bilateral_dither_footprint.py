"""GPU footprint of vszip_bilateral_dither: the "Plane memory" clauses of include/vszip_hip.h (readable extent, independence, written
extent) through the guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py uses, for both integer sample widths
and f32, both paths, with and without `ref`: guards, pitch padding, a window's live neighbours, every source, every `ref` plane and
every point table come back as uploaded; only `[0, w) x h` of each output is written and it equals the spec
(tests/bilateral_dither_ref.py) bit for bit; the runs with poison 0x00 and 0xFF around the planes give the same bits. The mirrored
halo never leaves `[0, w) x h`. The point table is a plane of the case like the sources (one row of 23 K pairs as 16-bit patterns), so its
footprint is watched too."""
import numpy as np
import pytest

import bilateral_dither_ref as bd
from test_gpu_footprint import LAYOUTS, Case, sizes_for

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.float32]
IDS = ["u8", "u16", "f32"]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _case(layout, seed, dtype, sizes, radius, subspl, with_ref):
    f = np.dtype(dtype) == np.float32
    bits = 32 if f else 8 * np.dtype(dtype).itemsize
    c = Case(layout, seed)
    d = bd.derive(f, bits, radius, 8.0, 0.4, 0.1, subspl)
    pts = bd.point_lists(radius, float(subspl)) if d["subsampled"] else None
    if pts is not None:
        flat = np.ascontiguousarray(pts).view(np.uint16).reshape(1, -1)
        c.add("pts", "in", np.uint16, 1, flat.shape[1], flat)
    planes = []
    for i, (h, w) in enumerate(sizes):
        a = np.ascontiguousarray(bd.noisy_plane(seed + i, h, w, dtype))
        r = np.ascontiguousarray(bd.noisy_plane(seed + i + 40, h, w, dtype)) if with_ref and i % 3 != 2 else None  # every third plane has no ref
        planes.append((a, r))
        c.add(f"src{i}", "in", dtype, h, w, a)
        if r is not None:
            c.add(f"ref{i}", "in", dtype, h, w, r)
        c.add(f"dst{i}", "out", dtype, h, w)
    return c, planes, d, pts, bits


def _run(dev, c, planes, d, pts, bits, radius, path):
    n = len(planes)

    def call(P):
        e = [dev.bilateral_dither_entry(radius, d["m"], d["wmax"], d["sum_w_min"], P.get("pts"), d["K"])] * n
        refs = [P.get(f"ref{i}") for i in range(n)]
        with dev.options(VSZIP_BILATERAL_DITHER_PATH=path):
            dev.bilateral_dither([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], e, refs if any(r is not None for r in refs) else None, bits)
    c.run(dev, call, {f"dst{i}": bd.plane(a, radius, d["m"], d["wmax"], d["sum_w_min"], bits, pts, r) for i, (a, r) in enumerate(planes)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("path", [1, 2], ids=["tile", "direct"])
@pytest.mark.parametrize("with_ref", [False, True], ids=["noref", "ref"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bilateral_dither(dev, dtype, with_ref, path, layout):
    sizes = sizes_for(layout, 37, 83, 3, 8, 8)
    dense = LAYOUTS.index(layout) % 2 == 0
    for radius, subspl in ((5, 2.0), (8, 0.0)) if dense else ((8, 0.0), (6, 4.0)):
        c, planes, d, pts, bits = _case(layout, 8, dtype, sizes, radius, subspl, with_ref)
        _run(dev, c, planes, d, pts, bits, radius, path)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_radius_beyond_the_tile_and_planes_as_small_as_the_radius(dev, dtype):
    c, planes, d, pts, bits = _case("odd_pad32", 4, dtype, [(45, 99), (40, 41)], 40, 0.0, True)
    _run(dev, c, planes, d, pts, bits, 40, 0)
    c, planes, d, pts, bits = _case("shift1", 5, dtype, [(16, 16), (16, 23), (29, 16)], 16, 2.0, True)
    _run(dev, c, planes, d, pts, bits, 16, 1)
