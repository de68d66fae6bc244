"""GPU: vszip_deband_lowbit, Deband on resident planes under 16 bits (up with dither none, vszip_deband's kernels, error-diffusion dither back).
The three 8-bit keys of the reference's Deband goldens (deband_ref.LEFT_OUT) through it, with the criterion those goldens allow (min and max equal,
|avg - golden| * w * h * peak < 0.5) and bit for bit against the numpy spec (tests/depth_ref.py); 8-, 10- and 12-bit YUV420 frames of 70 x 38 in sample
modes 2 and 7 with grain on and off, byte for byte equal to the three separate calls (depth, deband, depth) and to the spec; a scratch cap small
enough to force several plane groups; the argument errors."""
import numpy as np
import pytest

import deband_ref as db
import depth_ref as dr
import fixtures as fx
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


class Clip:
    """the per-clip state deband_ref.deband_frame derives from its keyword arguments, resident: tables, grain, and one entry per plane"""

    def __init__(self, dev, shapes, family, ssw, ssh, **kw):
        self.a = a = db.check_args(**kw)
        h, w = shapes[0]
        self.tab = tab = db.clip_tables(w, h, ssw, ssh, 1, False, a)
        self.rtab = dev.upload_deband_tables(tab)
        thr, thr1, thr2 = (db.scale_value(a[k], False) for k in ("thr", "thr1", "thr2"))
        yuv = family == "YUV"
        self.entries = []
        for i, (ph, pw) in enumerate(shapes):
            lo, hi = ((db.TV_C if i > 0 else db.TV_Y) if a["keep_tv_range"] and yuv else (0, 65535))
            grain = self.rtab["grain_y" if i == 0 else "grain_c"]
            off = int(tab["grain_offsets"][0]) if tab["grain_offsets"] is not None else 0
            self.entries.append(dev.deband_entry(self.rtab["luma" if i == 0 else "chroma"], ssw if i > 0 else 0, ssh if i > 0 else 0, grain, off,
                                                 db.grain_pitch(w if i == 0 else (w >> ssw), 2), thr[i], thr1[i], thr2[i], lo, hi))
        self.args = dict(sample_mode=a["sample_mode"], blur_first=a["blur_first"], angle_boost=a["angle_boost"], max_angle=a["max_angle"], max_offset=tab["max_offset"])


def lowbit(dev, clip, planes, bits, full=False, copies=1, **opts):
    srcs = [dev.upload(p) for _ in range(copies) for p in planes]
    dsts = [dev.empty(p.shape[0], p.shape[1], p.dtype) for _ in range(copies) for p in planes]
    with dev.options(**opts):
        dev.deband_lowbit(srcs, dsts, clip.entries * copies, bits, full, **clip.args)
    return [dev.download(d) for d in dsts]


def three_calls(dev, clip, planes, bits, full=False):
    srcs = [dev.upload(p) for p in planes]
    up, mid = ([dev.empty(p.shape[0], p.shape[1], np.uint16) for p in planes] for _ in range(2))
    dsts = [dev.empty(p.shape[0], p.shape[1], p.dtype) for p in planes]
    dev.depth(srcs, up, bits, 16, dr.NONE, full)
    dev.deband(up, mid, clip.entries, **clip.args)
    dev.depth(mid, dsts, 16, bits, dr.ERROR_DIFFUSION, full)
    return [dev.download(d) for d in dsts]


@pytest.mark.parametrize("key", sorted(db.LEFT_OUT))
def test_the_8_bit_goldens(dev, key):
    fmt, _, kw = db.parse_key(key)
    family, ssw, ssh = dr._FMT8[fmt]
    planes = dr.golden_inputs8(fmt)
    outs = lowbit(dev, Clip(dev, [p.shape for p in planes], family, ssw, ssh, **kw), planes, 8)
    for i, o in enumerate(outs):
        print(key, i, fx.plane_stats(o), db.goldens()[key][f"p{i}"])
    assert dr.same_as_golden(key, outs) == []
    for o, e in zip(outs, dr.run_key8(key)):
        assert o.dtype == np.uint8 and np.array_equal(o, e), int((o != e).sum())


def frame(bits, seed=0):
    """a YUV420 frame of 70 x 38 at `bits`: natural content with a little noise (thresholds decide both ways)"""
    out = []
    for i, (h, w) in enumerate([(38, 70), (19, 35), (19, 35)]):
        a = fx.tiled_natural((h, w), np.uint16, i) // 2 + (fx.splitmix64_plane(seed + i, (h, w), np.uint16) >> 6)
        out.append((a >> (16 - bits)).astype(dr.dtype_of(bits)))
    return out


@pytest.mark.parametrize("grain", [0, 16], ids=["no-grain", "grain"])
@pytest.mark.parametrize("mode", [2, 7])
@pytest.mark.parametrize("bits", [8, 10, 12])
def test_equal_to_the_three_separate_calls_and_to_the_spec(dev, bits, mode, grain):
    planes = frame(bits)
    kw = dict(thr=48, grain=grain, seed=7, sample_mode=mode)
    clip = Clip(dev, [p.shape for p in planes], "YUV", 1, 1, **kw)
    outs, apart, spec = lowbit(dev, clip, planes, bits), three_calls(dev, clip, planes, bits), dr.deband_lowbit_frame(planes, bits, "YUV", 1, 1, **kw)
    for i, (o, a, e, p) in enumerate(zip(outs, apart, spec, planes)):
        assert o.dtype == p.dtype and o.tobytes() == a.tobytes(), (i, int((o != a).sum()))
        assert np.array_equal(o, e), (i, int((o != e).sum()))
    assert any(not np.array_equal(o, p) for o, p in zip(outs, planes))


def test_full_range_gray(dev):
    p = [frame(10, 4)[0]]
    kw = dict(thr=48, grain=16, seed=3)
    clip = Clip(dev, [p[0].shape], "GRAY", 0, 0, **kw)
    out, spec = lowbit(dev, clip, p, 10, full=True)[0], dr.deband_lowbit_frame(p, 10, "GRAY", full_range=True, **kw)[0]
    assert np.array_equal(out, spec)


@pytest.mark.parametrize("mode", [2, 7])
def test_a_small_scratch_cap_forces_several_plane_groups(dev, mode):
    """four copies of a 320 x 160 YUV420P8 frame: two 16-bit intermediates of a luma plane are 200 KiB, of a chroma plane 50 KiB, so a cap of 1 MiB
    ends a group every few planes (and in mode 7 the angle planes' cap of 1 MiB, 200 KiB a luma plane, ends some earlier)"""
    planes = [np.ascontiguousarray(p[:160 >> (i > 0), :320 >> (i > 0)]) for i, p in enumerate(dr.golden_inputs8("YUV420P8"))]
    kw = dict(thr=48, grain=16, seed=7, sample_mode=mode)
    clip = Clip(dev, [p.shape for p in planes], "YUV", 1, 1, **kw)
    assert dev.get_option("VSZIP_DEBAND_LOWBIT_SCRATCH_MIB") == 1024
    spec = dr.deband_lowbit_frame(planes, 8, "YUV", 1, 1, **kw)
    one = lowbit(dev, clip, planes, 8, copies=4)
    capped = lowbit(dev, clip, planes, 8, copies=4, VSZIP_DEBAND_LOWBIT_SCRATCH_MIB=1, VSZIP_DEBAND_SCRATCH_MIB=1)
    for i, (o, c) in enumerate(zip(one, capped)):
        assert np.array_equal(o, spec[i % 3]) and np.array_equal(c, spec[i % 3]), i


def test_argument_errors(dev):
    p8 = frame(8)[:1]
    clip = Clip(dev, [p8[0].shape], "GRAY", 0, 0, thr=48)
    s, d = dev.upload(p8[0]), dev.empty(38, 70, np.uint8)
    for bits in (7, 16):
        with pytest.raises(VszipError, match=f"Deband: bits {bits} is outside 8..15"):
            # (the binding checks the sample type first: call the entry itself)
            dev.check(dev.lib.vszip_deband_lowbit(dev.ctx, bits, 0, dev.plane_table([s], [d]), (type(clip.entries[0]) * 1)(*clip.entries), 1, 2, 1, 1.5, 0.15, 15))
    with pytest.raises(VszipError, match=r'Deband: parameter "sample_mode=9" out of range \[1\.\.7\]\.'):
        dev.deband_lowbit([s], [d], clip.entries, 8, **dict(clip.args, sample_mode=9))
    with pytest.raises(VszipError, match="Depth: plane 0: bad geometry 70x38, pitches 72 -> 8"):
        dev.deband_lowbit([s], [dev.wrap(d.ptr, 38, 70, 8, np.uint8)], clip.entries, 8, **clip.args)
    with pytest.raises(ValueError, match="bits=10 takes uint16 planes"):
        dev.deband_lowbit([s], [d], clip.entries, 10, **clip.args)
    dev.deband_lowbit([s], [d], clip.entries, 8, **clip.args)  # and the valid call goes through
    assert np.array_equal(dev.download(d), dr.deband_lowbit_frame(p8, 8, "GRAY", thr=48)[0])
