"""GPU footprint of vszip_image_unpack: the "Plane memory" clause of include/vszip_hip.h (reads inside the w x pixel-bytes of each source
row, independence, written extent) through the guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py uses, for
rgb24, rgba32 with alpha, rgba64, float32, grey + alpha and INDEXED: guards, pitch padding, a window's live neighbours and the packed
source come back as uploaded; only `[0, w) x h` of each output plane is written and it equals the spec (tests/image_unpack_ref.py) bit
for bit; the runs with poison 0x00 and 0xFF around the planes give the same bits. The source is a plane of bytes, w x pixel-bytes wide,
so its pitch is in bytes as the entry point takes it, and in the odd layouts it starts at an odd byte whatever the sample type."""
import numpy as np
import pytest

import image_unpack_ref as iu
from test_gpu_footprint import LAYOUTS, Case, sizes_for

pytestmark = pytest.mark.gpu

COMBOS = {"rgb24": (iu.RGB, np.uint8, 8), "rgba32": (iu.RGBA, np.uint8, 8), "rgba64": (iu.RGBA, np.uint16, 16), "float32": (iu.RGBA, np.float32, 32),
          "gray8_alpha": (iu.GRAY_ALPHA, np.uint8, 8), "gray16_alpha": (iu.GRAY_ALPHA, np.uint16, 16), "indexed": (iu.INDEXED, np.uint8, 8)}


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _run(dev, layout, sizes, combo, seed, drop_alpha=False):
    lay, dt, bits = combo
    pxb = np.dtype(dt).itemsize * iu.CHANNELS[lay]
    pal = iu.palette(seed) if lay == iu.INDEXED else None
    ncol = 1 if lay in (iu.GRAY, iu.GRAY_ALPHA) else 3
    c = Case(layout, seed)
    expect = {}
    for i, (h, w) in enumerate(sizes):
        packed = iu.content(seed + i, h, w, combo)
        c.add(f"src{i}", "in", np.uint8, h, w * pxb, iu.row_bytes(packed))
        p, a = iu.unpack(packed, lay, bits, pal, alpha=not drop_alpha)
        for k, x in enumerate(p):
            c.add(f"p{k}_{i}", "out", dt, h, w)
            expect[f"p{k}_{i}"] = x
        if a is not None:
            c.add(f"a{i}", "out", dt, h, w)
            expect[f"a{i}"] = a
    n = len(sizes)

    def call(P):
        dev.image_unpack([P[f"src{i}"] for i in range(n)], [[P[f"p{k}_{i}"] for k in range(ncol)] for i in range(n)], [P.get(f"a{i}") for i in range(n)], lay, bits, pal)
    c.run(dev, call, expect)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(COMBOS))
def test_image_unpack(dev, name, layout):
    _run(dev, layout, sizes_for(layout, 37, 83, 2, 1, 1), COMBOS[name], 4)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(COMBOS))
def test_small_frames_and_whole_units(dev, name, layout):
    _run(dev, layout, [(1, 1), (7, 13), (2, 16), (3, 64), (5, 17)] if layout == "packed" else [(3, 5), (2, 64), (1, 16)], COMBOS[name], 7)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["rgba32", "float32", "indexed"])
def test_the_alpha_channel_dropped(dev, name, layout):
    _run(dev, layout, sizes_for(layout, 37, 83, 2, 1, 1), COMBOS[name], 5, drop_alpha=True)
