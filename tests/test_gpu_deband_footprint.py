"""GPU footprint of vszip_deband: the "Plane memory" clauses of include/vszip_hip.h (readable extent, independence, written
extent) through the guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py uses, for both sample
types and both gather paths: guards, pitch padding, a window's live neighbours, every source, every offset table and every
grain plane come back as uploaded; only `[0, w) x h` of each output is written and it equals the spec (tests/deband_ref.py)
bit for bit; the runs with poison 0x00 and 0xFF around the planes give the same bits. The tile path's four-sample staging
loads may cover pitch padding; what they bring lands in LDS columns that nothing reads. Tables and grain are planes of the
case like the sources, laid out the same way (shifted bases, odd pitches, windows), so their footprint is watched too."""
import numpy as np
import pytest

import deband_ref as db
from test_gpu_footprint import LAYOUTS, Case, content, sizes_for

pytestmark = pytest.mark.gpu

DTYPES = [np.uint16, np.float32]
IDS = ["u16", "f32"]
MODES = (2, 5, 7, 1, 3, 4, 6)


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _case(layout, seed, dtype, sizes, rng):
    f = np.dtype(dtype) == np.float32
    c = Case(layout, seed)
    planes = []
    for i, (h, w) in enumerate(sizes):
        a = content(seed + i, h, w, dtype, i % 2 == 0)
        if not f:
            a = (a >> 1) + 8000  # room for the grain on both sides of the clamp
        t = db.tables(w, h, range=rng, sample_mode=2, seed=seed + i, grain=(0.06, 0) if f else (4112, 0), is_float=f)
        g = np.ascontiguousarray(t["grain_y"][:h * w].reshape(h, w)) if i % 3 != 2 else None  # every third plane has no grain
        planes.append((a, t["luma"], g))
        c.add(f"src{i}", "in", dtype, h, w, a)
        # (tables and integer grain travel as their 16-bit patterns: the arena's layouts know unsigned samples)
        c.add(f"tab{i}", "in", np.uint16, h, w, np.ascontiguousarray(t["luma"]).view(np.uint16).reshape(h, w))
        if g is not None:
            c.add(f"gr{i}", "in", np.float32 if f else np.uint16, h, w, g if f else g.view(np.uint16))
        c.add(f"dst{i}", "out", dtype, h, w)
    return c, planes


def _run(dev, c, planes, dtype, mode, path, max_offset):
    f = np.dtype(dtype) == np.float32
    n = len(planes)
    thr = [tuple((48 + 16 * (i % 3)) * k / 255.0 for k in (1.0, 1.6, 0.4)) if f else tuple(int((48 + 16 * (i % 3)) * 257 * k) for k in (1.0, 1.6, 0.4)) for i in range(n)]
    lo, hi = (0.05, 0.9) if f else (9000, 38000)

    def call(P):
        e = [dev.deband_entry(P[f"tab{i}"], 0, 0, P.get(f"gr{i}"), 0, P[f"gr{i}"].stride if f"gr{i}" in P else 0, *thr[i], lo, hi) for i in range(n)]
        with dev.options(VSZIP_DEBAND_PATH=path):
            dev.deband([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], e, mode, True, 1.5, 0.15, max_offset)
    # (the table of a plane was made for mode 2: its second value is simply not used by the other modes)
    c.run(dev, call, {f"dst{i}": db.deband_plane(a, t, 0, 0, g, *thr[i], lo, hi, mode, True, 1.5, 0.15) for i, (a, t, g) in enumerate(planes)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("path", [1, 2], ids=["tile", "direct"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_deband(dev, dtype, path, layout):
    c, planes = _case(layout, 8, dtype, sizes_for(layout, 45, 203, 3, 4, 4), 15)
    _run(dev, c, planes, dtype, MODES[LAYOUTS.index(layout) % len(MODES)], path, 15)
    _run(dev, c, planes, dtype, MODES[(LAYOUTS.index(layout) + 3) % len(MODES)], path, 15)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_larger_halo_and_the_full_range(dev, dtype):
    """range 31 takes the tile path's 32-sample halo; range 255 (max_offset 128) the direct path"""
    c, planes = _case("odd_pad32", 4, dtype, [(99, 203), (70, 97)], 31)
    _run(dev, c, planes, dtype, 2, 1, 31)
    c, planes = _case("shift1", 5, dtype, [(280, 300)], 255)
    assert any((t == -128).any() for _, t, _ in planes)
    _run(dev, c, planes, dtype, 2, 0, 128)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tables_longer_than_one_launch(dev, dtype):
    """200 planes of differing sizes, packed back to back, every neighbour's guard watching: three launches"""
    c, planes = _case("packed", 23, dtype, [(4 + i % 11, 4 + i % 37) for i in range(200)], 3)
    _run(dev, c, planes, dtype, 2, 1, 3)
