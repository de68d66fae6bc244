"""GPU footprint of vszip_compress: the "Plane memory" clauses of include/vszip_hip.h (readable extent, independence, written extent)
through the guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py uses, for both codecs, with luma and chroma
tables mixed: guards, pitch padding, a window's live neighbours and every source come back as uploaded; only `[0, w) x h` of each
output is written and it equals the spec (tests/compress_ref.py) bit for bit; the runs with poison 0x00 and 0xFF around the planes
give the same bits, which pins the replication of a partial block's last column and row to in-plane samples."""
import numpy as np
import pytest

import compress_ref as cr
from test_gpu_footprint import LAYOUTS, Case, sizes_for
from vszip_amd import capi

pytestmark = pytest.mark.gpu

PARAMS = [cr.MPEG2_PARAMS[2], cr.MPEG2_PARAMS[5], cr.JPEG_PARAMS[1], cr.JPEG_PARAMS[2]]
IDS = [",".join(f"{k}={v}" for k, v in kw.items()) for kw in PARAMS]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _run(dev, layout, sizes, kw, seed, in_place=False):
    a = dict(cr.DEFAULTS, **kw)
    spec_tb, lib_tb = cr.tables(**a), capi.compress_tables(**a)
    c = Case(layout, seed)
    planes, chroma = [], [bool(i & 1) for i in range(len(sizes))]
    for i, (h, w) in enumerate(sizes):
        p = cr.gpu_plane(seed + i, w, h)
        planes.append(p)
        if in_place:
            c.add(f"dst{i}", "inout", np.uint8, h, w, p)
        else:
            c.add(f"src{i}", "in", np.uint8, h, w, p)
            c.add(f"dst{i}", "out", np.uint8, h, w)
    n = len(planes)

    def call(P):
        dev.compress([P[f"dst{i}" if in_place else f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], lib_tb, chroma)
    c.run(dev, call, {f"dst{i}": cr.plane(p, spec_tb, chroma[i]) for i, p in enumerate(planes)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kw", PARAMS, ids=IDS)
def test_compress(dev, kw, layout):
    _run(dev, layout, sizes_for(layout, 37, 83, 3, 1, 1), kw, 4)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_planes_of_less_than_a_block_and_whole_blocks(dev, layout):
    for kw in (PARAMS[0], PARAMS[3]):
        _run(dev, layout, [(1, 1), (13, 7), (8, 8), (16, 24), (9, 9)] if layout == "packed" else [(3, 5), (16, 24), (8, 16)], kw, 7)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_in_place(dev, layout):
    """dst == src: same pointer, same stride"""
    for kw in (PARAMS[1], PARAMS[2]):
        _run(dev, layout, sizes_for(layout, 37, 83, 3, 1, 1), kw, 5, in_place=True)
