"""GPU footprint of vszip_comb_mask / vszip_comb_mask_mt: the three "Plane memory" clauses of include/vszip_hip.h
(readable extent, independence, written extent) through the guarded arena (tests/guarded.py), over the layouts
tests/test_gpu_footprint.py uses for AdaptiveBinarize: guards, pitch padding, a window's live neighbours and every
input come back as uploaded; `[0, w) x h` of each mask equals the spec (tests/combmask_ref.py); the runs with poison
0x00 and 0xFF around the planes give the same bits. The reference writes and reads the pitch padding; this library
does not."""
import numpy as np
import pytest

import combmask_ref as cr
import fixtures as fx
from test_gpu_footprint import LAYOUTS, Case, content, sizes_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _case(layout, seed, with_prev):
    c = Case(layout, seed)
    sizes = sizes_for(layout, 45, 203, 1, 9, 9)
    srcs, prvs = [], []
    for i, (h, w) in enumerate(sizes):
        s = content(seed + i, h, w, np.uint8, i % 2 == 0)
        s[1::2] = np.clip(s[1::2].astype(np.int32) + 30, 0, 255).astype(np.uint8)  # combing
        p = s.copy()
        mov = fx.splitmix64_plane(500 + seed + i, (h, w), np.uint8) > 128
        p[mov] = 255 - p[mov]
        srcs.append(s)
        prvs.append(p)
        c.add(f"src{i}", "in", np.uint8, h, w, s)
        if with_prev:
            c.add(f"prv{i}", "in", np.uint8, h, w, p)
        c.add(f"dst{i}", "out", np.uint8, h, w)
    return c, srcs, prvs


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("expand", [False, True], ids=["plain", "expand"])
@pytest.mark.parametrize("mthresh", [0, 9], ids=["spatial", "motion"])
def test_comb_mask(dev, mthresh, expand, metric, layout):
    c, srcs, prvs = _case(layout, 6, mthresh > 0)
    n = len(srcs)

    def call(P):
        g = lambda r: [P[f"{r}{i}"] for i in range(n)]
        dev.comb_mask(g("src"), g("dst"), g("prv") if mthresh else None, cthresh=6, mthresh=mthresh, expand=expand, metric=metric)
    c.run(dev, call, {f"dst{i}": cr.comb_mask(srcs[i], prvs[i], 6, mthresh, expand, metric) for i in range(n)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("thy", [(30, 30), (10, 90)], ids=["binary", "gradient"])
def test_comb_mask_mt(dev, thy, layout):
    c, srcs, _ = _case(layout, 7, False)
    n = len(srcs)

    def call(P):
        dev.comb_mask_mt([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], *thy)
    c.run(dev, call, {f"dst{i}": cr.comb_mask_mt(srcs[i], *thy) for i in range(n)})


@pytest.mark.parametrize("filt", ["comb_mask", "comb_mask_mt"])
def test_tables_longer_than_one_launch(dev, filt):
    """200 planes of differing sizes, packed back to back in shuffled order, every neighbour's guard watching"""
    n = 200
    c = Case("packed", 19)
    srcs, prvs = [], []
    for i in range(n):
        h, w = 9 + i % 11, 17 + i % 37
        srcs.append(content(i, h, w, np.uint8, i % 4 == 0))
        prvs.append(content(1000 + i, h, w, np.uint8, False))
        c.add(f"src{i}", "in", np.uint8, h, w, srcs[i])
        c.add(f"prv{i}", "in", np.uint8, h, w, prvs[i])
        c.add(f"dst{i}", "out", np.uint8, h, w)
    g = lambda P, r: [P[f"{r}{i}"] for i in range(n)]
    if filt == "comb_mask":
        call = lambda P: dev.comb_mask(g(P, "src"), g(P, "dst"), g(P, "prv"), cthresh=3, mthresh=20)
        want = [cr.comb_mask(s, p, 3, 20) for s, p in zip(srcs, prvs)]
    else:
        call = lambda P: dev.comb_mask_mt(g(P, "src"), g(P, "dst"), 5, 60)
        want = [cr.comb_mask_mt(s, 5, 60) for s in srcs]
    c.run(dev, call, {f"dst{i}": w for i, w in enumerate(want)})
