"""GPU footprint of vszip_mosquito_nr: the "Plane memory" clauses of include/vszip_hip.h (readable extent, independence,
written extent) through the guarded arena (tests/guarded.py), over the layouts tests/test_gpu_footprint.py uses, for the
three sample types: guards, pitch padding, a window's live neighbours and every source come back as uploaded; only
`[0, w) x h` of each output is written and it equals the spec (tests/mosquito_ref.py) bit for bit; the runs with poison
0x00 and 0xFF around the planes give the same bits. A workgroup's four-sample loads may cover pitch padding; what they
bring lands in LDS columns that nothing reads."""
import numpy as np
import pytest

import mosquito_ref as mq
from test_gpu_footprint import LAYOUTS, Case, content, sizes_for

pytestmark = pytest.mark.gpu

DTYPES = [(np.uint8, 8), (np.uint16, 16), (np.float32, 32)]
IDS = ["u8", "u16", "f32"]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _case(layout, seed, dtype, sizes, natural_every=2):
    c = Case(layout, seed)
    datas = []
    for i, (h, w) in enumerate(sizes):
        a = content(seed + i, h, w, dtype, i % natural_every == 0)
        datas.append(a)
        c.add(f"src{i}", "in", dtype, h, w, a)
        c.add(f"dst{i}", "out", dtype, h, w)
    return c, datas


def _params(n):
    """per-plane parameters that differ within the call: both radii, every kind of restore, a copied plane"""
    return ([(16, 32, 0, 8, 24)[i % 5] for i in range(n)], [(128, 64, 128, 0, 127)[i % 5] for i in range(n)], [2 - i % 2 for i in range(n)], [i % 3 == 1 for i in range(n)])


def _run(dev, c, datas, bits):
    n = len(datas)
    st, rs, rd, ch = _params(n)
    b = None if bits == 32 else bits

    def call(P):
        dev.mosquito_nr([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], st, rs, rd, b, ch)
    c.run(dev, call, {f"dst{i}": mq.mosquito_nr(a, st[i], rs[i], rd[i], b, ch[i]) for i, a in enumerate(datas)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype,bits", DTYPES, ids=IDS)
def test_mosquito_nr(dev, dtype, bits, layout):
    c, datas = _case(layout, 8, dtype, sizes_for(layout, 45, 203, 3, 4, 4))
    _run(dev, c, datas, bits)


@pytest.mark.parametrize("dtype,bits", DTYPES, ids=IDS)
def test_tables_longer_than_one_launch(dev, dtype, bits):
    """200 planes of differing sizes, packed back to back, every neighbour's guard watching: two launches"""
    c, datas = _case("packed", 23, dtype, [(4 + i % 11, 4 + i % 37) for i in range(200)], natural_every=4)
    _run(dev, c, datas, bits)
