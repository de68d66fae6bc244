"""GPU footprint of vszip_pack_rgb: the "Plane memory" clauses of include/vszip_hip.h (readable extent, independence, written extent)
through the guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py uses, for RGB24 and RGB30: guards, pitch
padding, a window's live neighbours and every input come back as uploaded; only `[0, w) x h` of each packed plane is written and it
equals the spec (tests/pack_rgb_ref.py) bit for bit; the runs with poison 0x00 and 0xFF around the planes give the same bits."""
import numpy as np
import pytest

import pack_rgb_ref as pr
from test_gpu_footprint import LAYOUTS, Case, sizes_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _run(dev, layout, sizes, bits, seed, one_input=False):
    dt = np.uint8 if bits == 8 else np.uint16
    c = Case(layout, seed)
    frames = []
    for i, (h, w) in enumerate(sizes):
        f = pr.gpu_frame(seed + i, w, h, bits)
        if one_input:
            f = [f[0]] * 3
            c.add(f"r{i}", "in", dt, h, w, f[0])
        else:
            for name, p in zip("rgb", f):
                c.add(f"{name}{i}", "in", dt, h, w, p)
        c.add(f"dst{i}", "out", np.uint32, h, w)
        frames.append(f)
    n = len(frames)

    def call(P):
        pick = lambda name: [P[f"{'r' if one_input else name}{i}"] for i in range(n)]
        dev.pack_rgb(pick("r"), pick("g"), pick("b"), [P[f"dst{i}"] for i in range(n)], bits)
    c.run(dev, call, {f"dst{i}": pr.pack(*f, bits) for i, f in enumerate(frames)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits", [8, 10])
def test_pack_rgb(dev, bits, layout):
    _run(dev, layout, sizes_for(layout, 37, 83, 3, 1, 1), bits, 4)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits", [8, 10])
def test_small_frames_and_whole_groups(dev, bits, layout):
    _run(dev, layout, [(1, 1), (7, 13), (2, 16), (3, 64), (5, 17)] if layout == "packed" else [(3, 5), (2, 64), (1, 16)], bits, 7)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_r_g_and_b_as_one_plane(dev, layout):
    for bits in (8, 10):
        _run(dev, layout, sizes_for(layout, 37, 83, 3, 1, 1), bits, 5, one_input=True)
