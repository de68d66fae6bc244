"""GPU: vszip_deband against the numpy spec (tests/deband_ref.py), bit for bit in both sample types: every sample mode, both
blur_first values, grain on and off, both gather paths forced (VSZIP_DEBAND_PATH), planes of several tiles and of less than one,
range 255 with wrapped (-128) entries on the direct path, chroma planes that share a table with a luma plane, per-plane
parameters, the grain of three frames in one call, unaligned bases and odd pitches, tables longer than one launch and angle
planes beyond the scratch cap, and a table with entries beyond the declared max_offset on the tile path inside the guarded
arena. The tables come from the spec; tests/test_deband_ref.py shows the library's generator makes the same bytes."""
from functools import lru_cache

import numpy as np
import pytest

import deband_ref as db
import fixtures as fx
import guarded as G
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu

TILE, DIRECT = 1, 2
DTYPES = [np.uint16, np.float32]
IDS = ["u16", "f32"]
SIZES = [(45, 203), (131, 97), (7, 13)]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


@lru_cache(maxsize=None)
def plane(seed, h, w, dtype):
    """natural content with a little noise: thresholds decide both ways"""
    a, n = fx.tiled_natural((h, w), dtype, seed % 3), fx.splitmix64_plane(seed, (h, w), dtype)
    p = (a // 2 + (n >> 6)).astype(np.uint16) if np.dtype(dtype) == np.uint16 else (a * np.float32(0.5) + n * np.float32(0.02)).astype(np.float32)
    p.setflags(write=False)
    return p


@lru_cache(maxsize=None)
def tables(w, h, mode, is_float, rng=15, ssw=0, ssh=0, seed=5, frames=1, dynamic=False):
    return db.tables(w, h, ssw, ssh, frames, rng, mode, seed, grain=(0.06, 0.03) if is_float else (4112, 2056), dynamic_grain=dynamic, is_float=is_float)


def thr_of(dtype, scale=1.0):
    f = np.dtype(dtype) == np.float32
    return tuple(v * scale / 255.0 for v in (48, 80, 20)) if f else tuple(int(v * 257 * scale) for v in (48, 80, 20))


def item(src, tab, chroma=False, ssw=0, ssh=0, grain=None, goff=0, gpitch=None, thr=None, lo=None, hi=None):
    f = src.dtype == np.float32
    t = thr if thr is not None else thr_of(src.dtype)
    return dict(src=src, table=tab["chroma" if chroma else "luma"], ssw=ssw, ssh=ssh, grain=grain, goff=goff,
                gpitch=gpitch if gpitch is not None else db.grain_pitch(src.shape[1], src.itemsize), thr=t,
                lo=lo if lo is not None else (0.0 if f else 4096), hi=hi if hi is not None else (1.0 if f else 60160))


def expected(it, mode, blur_first=True, ab=1.5, ma=0.15):
    h, w = it["src"].shape
    g = db.grain_plane(it["grain"], it["goff"], it["gpitch"], h, w) if it["grain"] is not None else None
    return db.deband_plane(it["src"], it["table"], it["ssw"], it["ssh"], g, *it["thr"], it["lo"], it["hi"], mode, blur_first, ab, ma)


def run(dev, items, mode, blur_first=True, ab=1.5, ma=0.15, max_offset=15, path=0, **opts):
    """one vszip_deband over all items -> the outputs; tables and grain buffers are uploaded once per array"""
    up = {}

    def resident(a, as_pairs):
        if id(a) not in up:
            up[id(a)] = dev.upload(np.ascontiguousarray(a).view(np.int16).reshape(a.shape[0], a.shape[1]) if as_pairs else a.reshape(1, -1))
        return up[id(a)]
    srcs = [dev.upload(it["src"]) for it in items]
    dsts = [dev.empty(it["src"].shape[0], it["src"].shape[1], it["src"].dtype) for it in items]
    entries = [dev.deband_entry(resident(it["table"], True), it["ssw"], it["ssh"], resident(it["grain"], False) if it["grain"] is not None else None, it["goff"],
                                it["gpitch"], *it["thr"], it["lo"], it["hi"]) for it in items]
    with dev.options(VSZIP_DEBAND_PATH=path, **opts):
        dev.deband(srcs, dsts, entries, mode, blur_first, ab, ma, max_offset)
    return [dev.download(d) for d in dsts]


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def check(dev, items, mode, **kw):
    spec = {k: kw[k] for k in ("blur_first", "ab", "ma") if k in kw}
    outs = run(dev, items, mode, **kw)
    for i, (it, o) in enumerate(zip(items, outs)):
        e = expected(it, mode, **spec)
        assert same(o, e), (i, it["src"].shape, mode, kw, int((o != e).sum()))
    return outs


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
@pytest.mark.parametrize("mode", range(1, 8))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_modes_and_paths(dev, dtype, mode, path):
    f = np.dtype(dtype) == np.float32
    for blur_first in (True, False):
        for with_grain in (False, True):
            items = []
            for k, (h, w) in enumerate(SIZES):
                t = tables(w, h, mode, f)
                items.append(item(plane(3 + k, h, w, dtype), t, grain=t["grain_y"] if with_grain else None))
            check(dev, items, mode, blur_first=blur_first, path=path)


@pytest.mark.parametrize("path", [0, TILE], ids=["auto", "tile-does-not-fit"])
@pytest.mark.parametrize("mode", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_range_255_with_wrapped_entries_goes_the_direct_path(dev, dtype, mode, path):
    f = np.dtype(dtype) == np.float32
    t = tables(300, 280, mode, f, rng=255, seed=0)
    assert (t["luma"] == -128).any() and t["max_offset"] == 128
    check(dev, [item(plane(9, 280, 300, dtype), t, grain=t["grain_y"])], mode, max_offset=128, path=path, ab=4.0, ma=0.5)


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
@pytest.mark.parametrize("ssw,ssh", [(1, 1), (1, 0)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_chroma_planes_share_the_table_of_their_luma_plane(dev, dtype, ssw, ssh, path):
    f = np.dtype(dtype) == np.float32
    H, W = 90, 202
    ch, cw = H >> ssh, W >> ssw
    for mode in (1, 2, 3, 5, 7):
        t = tables(W, H, mode, f, ssw=ssw, ssh=ssh)
        assert t["chroma"].shape[:2] == (ch, cw)
        items = [item(plane(1, H, W, dtype), t, grain=t["grain_y"]),
                 item(plane(2, ch, cw, dtype), t, True, ssw, ssh, grain=t["grain_c"], lo=-0.5 if f else 4096, hi=0.5 if f else 61440),
                 item(plane(4, ch, cw, dtype), t, True, ssw, ssh, grain=t["grain_c"], lo=-0.5 if f else 4096, hi=0.5 if f else 61440)]
        if f:
            items[1]["src"] = items[1]["src"] - np.float32(0.3)
        check(dev, items, mode, path=path)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_per_plane_parameters_differ_within_a_call(dev, dtype):
    f = np.dtype(dtype) == np.float32
    for mode in (2, 5, 6):
        t = tables(97, 131, mode, f)
        src = plane(6, 131, 97, dtype)
        items = [item(src, t, grain=t["grain_y"], thr=thr_of(dtype, s), lo=lo, hi=hi)
                 for s, lo, hi in ((1.0, None, None), (0.25, 0.2 if f else 20000, 0.4 if f else 30000), (3.0, 0.0, 1.0 if f else 65535), (0.0, None, None))]
        outs = check(dev, items, mode, path=TILE)
        assert not same(outs[0], outs[1]) and not same(outs[0], outs[2]) and not same(outs[0], outs[3])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_call_uses_the_grain_of_three_frames(dev, dtype):
    f = np.dtype(dtype) == np.float32
    t = tables(203, 45, 2, f, frames=3, dynamic=True)
    offs = [int(o) for o in t["grain_offsets"]]
    assert len(set(offs)) == 3 and all(o % 16 == 0 for o in offs)
    src = plane(3, 45, 203, dtype)
    for path in (TILE, DIRECT):
        outs = check(dev, [item(src, t, grain=t["grain_y"], goff=o) for o in offs], 2, path=path)
        assert not same(outs[0], outs[1]) and not same(outs[1], outs[2])


@pytest.mark.parametrize("path", [TILE, DIRECT], ids=["tile", "direct"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_bases_and_odd_pitches_give_the_same_bits(dev, dtype, path):
    """every pointer one element off a 16-byte boundary and every pitch odd, each in turn and all together"""
    f = np.dtype(dtype) == np.float32
    h, w = 45, 203
    keep = []

    def shifted(a, shift, pitch):
        a = np.ascontiguousarray(a)
        big = dev.empty(a.shape[0] + 1, pitch + 32, a.dtype)
        keep.append(big)
        v = dev.wrap(big.ptr + shift * a.itemsize, a.shape[0], a.shape[1], pitch, a.dtype)
        dev.copy_in(v, a)
        dev.sync()
        return v
    src = plane(3, h, w, dtype)
    for mode in (2, 7):
        t = tables(w, h, mode, f)
        gp = db.grain_pitch(w, src.itemsize)
        it = item(src, t, grain=t["grain_y"])
        want = expected(it, mode)
        pairs = t["luma"].view(np.int16).reshape(h, w)
        g2 = np.ascontiguousarray(db.grain_plane(t["grain_y"], 0, gp, h, w))
        for which in ("src", "dst", "table", "grain", "all"):
            on = lambda k: which in (k, "all")
            s = shifted(src, 1 if on("src") else 0, 211 if on("src") else 224)
            d = dev.wrap(shifted(np.zeros_like(src), 1 if on("dst") else 0, 213 if on("dst") else 224).ptr, h, w, 213 if on("dst") else 224, dtype)
            tb = shifted(pairs, 1 if on("table") else 0, 205 if on("table") else 224)
            gr = shifted(g2, 1 if on("grain") else 0, 207 if on("grain") else 224)
            e = dev.deband_entry(tb, 0, 0, gr, 0, gr.stride, *it["thr"], it["lo"], it["hi"])
            with dev.options(VSZIP_DEBAND_PATH=path):
                dev.deband([s], [d], [e], mode, True, 1.5, 0.15, 15)
            assert same(dev.download(d), want), (mode, which)
    dev.sync()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tables_longer_than_one_launch_and_angle_planes_beyond_the_scratch_cap(dev, dtype):
    """200 planes: three launches of the 96-entry table; in mode 7 with a 1 MiB cap the 40 x 600 planes (94 KiB of angles each) run
    in groups of ten"""
    f = np.dtype(dtype) == np.float32
    small = [(4 + i % 11, 4 + i % 37) for i in range(200)]
    tabs = {s: tables(s[1], s[0], 2, f, rng=3) for s in set(small)}
    check(dev, [item(plane(i, h, w, dtype), tabs[(h, w)], grain=tabs[(h, w)]["grain_y"]) for i, (h, w) in enumerate(small)], 2, max_offset=3)
    t7 = tables(600, 40, 7, f)
    assert dev.get_option("VSZIP_DEBAND_SCRATCH_MIB") == 1024
    check(dev, [item(plane(i, 40, 600, dtype), t7) for i in range(25)], 7, VSZIP_DEBAND_SCRATCH_MIB=1)


def test_mode_7_takes_the_boost_branch_for_some_samples_and_not_for_others():
    """on the spec's own mask, for the inputs the mode 7 cases above use (checked on the CPU)"""
    for dtype in DTYPES:
        f = np.dtype(dtype) == np.float32
        for k, (h, w) in enumerate(SIZES[:2]):
            m = db.boost_mask(plane(3 + k, h, w, dtype), tables(w, h, 7, f)["luma"], 0, 0, 0.15)
            assert 0.02 < m.mean() < 0.98, (dtype, h, w, m.mean())


@pytest.mark.parametrize("declared", [15, 128], ids=["declared-15-tile", "declared-128"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_entries_beyond_the_halo_stay_inside_the_planes(dev, dtype, declared):
    """An otherwise valid range-15 table with a few entries raised to 100, 127 and -128. Declared 15, the call takes the tile path, whose
    gathers are clamped into the staged rectangle; declared 128 ("accordingly"), the tile does not fit and the direct path clamps into the
    plane. Either way every sample whose entry is untouched equals the spec, and the guarded arena sees no write outside the outputs
    (a read outside the allocation would fault; one inside it that mattered would differ between the two poisons)."""
    from test_gpu_footprint import Case

    f = np.dtype(dtype) == np.float32
    h, w = 77, 150
    src = plane(5, h, w, dtype)
    for mode in (2, 4):
        t = tables(w, h, mode, f)
        tab = t["luma"].copy()
        touched = np.zeros((h, w), bool)
        for (y, x, v) in [(0, 0, 100), (3, 149, 127), (76, 5, -128), (40, 70, 127), (31, 63, -128), (32, 64, 100), (76, 149, 127)]:
            tab[y, x] = (v, v if mode == 2 else 0)
            touched[y, x] = True
        it = item(src, dict(luma=t["luma"]))
        want = expected(it, mode)
        c = Case("odd_pad32", 3)
        c.add("src", "in", dtype, h, w, np.ascontiguousarray(src))
        c.add("tab", "in", np.uint16, h, w, np.ascontiguousarray(tab).view(np.uint16).reshape(h, w))
        c.add("dst", "out", dtype, h, w)

        def call(arena):
            P = {s.name: dev.wrap(arena.address(s.name), s.h, s.w, s.pitch, s.dtype) for s in arena.specs}
            with dev.options(VSZIP_DEBAND_PATH=TILE):
                dev.deband([P["src"]], [P["dst"]], [dev.deband_entry(P["tab"], 0, 0, None, 0, 0, *it["thr"], it["lo"], it["hi"])], mode, True, 1.5, 0.15, declared)
            dev.sync()
        outs, _ = G.run_case(lambda: G.DeviceBackend(dev), c.make_specs, call, {"dst": want}, same=lambda name, g, e: np.array_equal(g[~touched], e[~touched]))
        assert np.array_equal(outs["dst"][~touched], want[~touched])


def test_argument_errors(dev):
    src = dev.upload(np.zeros((8, 8), np.uint16))
    dst = dev.empty(8, 8, np.uint16)
    tab = dev.upload(np.zeros((8, 8), np.int16))
    e = [dev.deband_entry(tab, thr=100)]
    for kw, msg in [(dict(sample_mode=8), r'Deband: parameter "sample_mode=8" out of range \[1\.\.7\]\.'),
                    (dict(sample_mode=0), r'Deband: parameter "sample_mode=0" out of range \[1\.\.7\]\.'),
                    (dict(angle_boost=-1.0), r'Deband: parameter "angle_boost=-1" out of range \[0\.\.65535\]\.'),
                    (dict(angle_boost=70000.0), r'Deband: parameter "angle_boost=70000" out of range \[0\.\.65535\]\.'),
                    (dict(max_angle=2.0), r'Deband: parameter "max_angle=2" out of range \[0\.\.1\]\.'),
                    (dict(max_angle=-0.5), r'Deband: parameter "max_angle=-0.5" out of range \[0\.\.1\]\.'),
                    (dict(max_offset=129), "max_offset 129")]:
        with pytest.raises(VszipError, match=msg):
            dev.deband([src], [dst], e, **kw)
    s8 = dev.upload(np.zeros((8, 8), np.uint8))
    with pytest.raises(VszipError, match="16-bit integer or 32-bit float"):
        dev.deband([s8], [dev.empty(8, 8, np.uint8)], e)
    dev.deband([src], [dst], e)  # and the valid call goes through
    assert not dev.download(dst).any()
