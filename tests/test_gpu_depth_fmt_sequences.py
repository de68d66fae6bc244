"""GPU: vszip_depth_fmt between two other entry points on one context, queued with no host synchronise in between (the pattern of
tests/test_gpu_call_sequences.py): neither neighbour's result changes, and the conversion's own does not depend on what ran before. The
neighbours are chosen for the state they share with it: vszip_depth's error diffusion with its carry row in the context's scratch (the same
region vszip_depth_fmt's carry row takes) and vszip_boxblur."""
import numpy as np
import pytest

import depth_fmt_ref as df
import depth_ref as dr
import fixtures as fx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("tin,tout,dither,size", [((df.F32, 32), (df.U8, 8), 1, (260, 4100)), ((df.U8, 8), (df.F32, 32), 0, (70, 203)), ((df.F32, 32), (df.F16, 16), 0, (70, 203))],
                         ids=["f32-u8-diffuse-scratch", "u8-f32", "f32-f16"])
def test_a_conversion_between_two_other_calls_changes_neither(dev, tin, tout, dither, size):
    h, w = size
    src = df.content(11, h, w, 8, True) if df.is_float(tin[0]) else dr.content(11, h, w, 8)
    a16, b16 = dr.content(12, 260, 4100, 16), fx.splitmix64_plane(13, (90, 333), np.uint16)
    with dev.options(VSZIP_DEPTH_WAVES=4):  # 260 rows on four waves: the carry row of 4100 columns is in scratch
        s, d = dev.upload(src), dev.empty(h, w, df.NP[tout[0]])
        sa, da = dev.upload(a16), dev.empty(260, 4100, np.uint8)
        sb, db = dev.upload(b16), dev.empty(90, 333, np.uint16)
        first = lambda: dev.depth([sa], [da], 16, 8, dr.ERROR_DIFFUSION)
        mid = lambda: dev.depth_fmt([s], [d], *tin, *tout, dither, True)
        last = lambda: dev.boxblur([sb], [db], 3, 2, 2, 1)
        alone = []
        for call, out in ((first, da), (mid, d), (last, db)):  # each alone, synchronised
            call()
            alone.append(dev.download(out))
        for out in (da, d, db):
            dev.copy_in(out, np.zeros((out.h, out.w), out.dtype))
        dev.sync()
        first(), mid(), last(), mid(), first()  # back to back
        dev.sync()
        for out, want in zip((da, d, db), alone):
            got = dev.download(out)
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), out.dtype
    assert np.array_equal(alone[0], dr.convert(a16, 16, 8, dr.ERROR_DIFFUSION))
    e = df.convert(src, *tin, *tout, dither, True)
    assert np.array_equal(alone[1].view(np.uint8), np.ascontiguousarray(e).view(np.uint8))
