"""GPU footprint of vszip_checkmate: the three "Plane memory" clauses of include/vszip_hip.h (readable extent,
independence, written extent) through the guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py
uses: guards, pitch padding, a window's live neighbours and every input (the neighbouring frames' planes included) come
back as uploaded; `[0, w) x h` of each output equals the spec (tests/checkmate_ref.py); the runs with poison 0x00 and
0xFF around the planes give the same bits. The reference copies two whole pitches at either end of a plane, padding
included; this library does not."""
import numpy as np
import pytest

import checkmate_ref as ck
import fixtures as fx
from test_gpu_footprint import LAYOUTS, Case, content, sizes_for

pytestmark = pytest.mark.gpu

ROLES = ("p2", "p1", "src", "n1", "n2")


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _frames(seed, h, w, natural):
    """five frames a few levels apart: with tthr2 = 8 both branches are taken"""
    base = content(seed, h, w, np.uint8, natural).astype(np.int32)
    return [np.clip(base + fx.splitmix64_plane(700 + seed + k, (h, w), np.uint8).astype(np.int32) % 13 - 6, 0, 255).astype(np.uint8) for k in range(5)]


def _add(c, i, frames, temporal):
    h, w = frames[2].shape
    for r, a in zip(ROLES, frames):
        if temporal or r not in ("p2", "n2"):
            c.add(f"{r}{i}", "in", np.uint8, h, w, a)
    c.add(f"dst{i}", "out", np.uint8, h, w)


def _call(dev, n, temporal, **kw):
    def call(P):
        g = lambda r: [P[f"{r}{i}"] for i in range(n)]
        dev.checkmate(g("src"), g("dst"), g("p1"), g("n1"), g("p2") if temporal else None, g("n2") if temporal else None, **kw)
    return call


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tthr2", [0, 8], ids=["spatial", "temporal"])
def test_checkmate(dev, tthr2, layout):
    c = Case(layout, 6)
    sets = [_frames(6 + i, h, w, i % 2 == 0) for i, (h, w) in enumerate(sizes_for(layout, 45, 203, 1, 9, 9))]
    for i, f in enumerate(sets):
        _add(c, i, f, tthr2 > 0)
    c.run(dev, _call(dev, len(sets), tthr2 > 0, thr=12, tmax=12, tthr2=tthr2), {f"dst{i}": ck.checkmate(*f, 12, 12, tthr2) for i, f in enumerate(sets)})


@pytest.mark.parametrize("tthr2", [0, 8], ids=["spatial", "temporal"])
def test_tables_longer_than_one_launch(dev, tthr2):
    """200 planes of differing sizes, packed back to back, every neighbour's guard watching"""
    n = 200
    c = Case("packed", 19)
    sets = [_frames(i, 9 + i % 11, 17 + i % 37, i % 4 == 0) for i in range(n)]
    for i, f in enumerate(sets):
        _add(c, i, f, tthr2 > 0)
    c.run(dev, _call(dev, n, tthr2 > 0, thr=3, tmax=20, tthr2=tthr2), {f"dst{i}": ck.checkmate(*f, 3, 20, tthr2) for i, f in enumerate(sets)})
