"""GPU footprint: every entry point that takes planes touches only what include/vszip_hip.h ("Plane memory: what a
call reads and writes") says it may. One matrix, filter x layout x type; every case goes through the guarded arena
(tests/guarded.py) twice, with poison 0x00 and 0xFF around and between the planes:

  * guards, pitch padding, the live neighbours of a window and every input come back byte for byte as uploaded;
  * `[0, w) x h` of each output equals the oracle under the rule of the filter's own test module (every pixel filter
    here is bit-exact; scalars: integers exact, float sums rel 1e-12 as tests/test_gpu_planestats.py, SSIMULACRA2
    abs 1e-7 as tests/test_gpu_ssimulacra2.py);
  * outputs and scalars of the two runs are bit-identical (no value depends on a byte outside the inputs' `[0, w) x h`).

A layout the library does not accept must be refused with an error code, which the case then asserts (with every plane
coming back untouched). Every base alignment and every pitch >= w is accepted, on a slower path where the vector path
needs alignment; the refusals in the matrix are EEDI3H without dh on the odd-width layouts (createImpl's mod-2 rule) and
the RT integer row pass over unaligned rows longer than 16000 samples.
No plane here is placed at the end of an allocation: reads whose value is thrown away are bounded by reading the
kernels ("Furthest read of every kernel"), not by running them against an unmapped page."""
import numpy as np
import pytest

import fixtures as fx
import guarded as G
from vszip_amd.capi import ERR_ARG, ERR_UNSUPPORTED, VszipError

pytestmark = pytest.mark.gpu

LAYOUTS = ["aligned16", "odd_pad32", "tight_odd", "shift1", "window", "packed"]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _up(n, a):
    return -(-n // a) * a


def lw(layout, w, even=False):
    """the width a layout asks for: whole 16-sample groups, or odd (even = True: the plane has half-width chroma; 2 x odd)"""
    if layout == "aligned16":
        return max(16, w // 16 * 16) if not even else max(32, w // 32 * 32)
    if layout == "packed":
        return w
    return ((w - 1) | 1) if not even else 2 * (((w // 2) - 1) | 1)


def sizes_for(layout, h, w, n=1, min_h=1, min_w=1):
    """n planes of the nominal size, or (packed) five or more of different sizes"""
    if layout != "packed":
        return [(h, lw(layout, w))] * n
    var = [(h, w), (max(min_h, h - 7), w + 9), (max(min_h, h // 2 + 1), max(min_w, w // 2 + 3)), (h + 3, max(min_w, w - 5)), (max(min_h, h // 2), max(min_w, w // 2)), (h + 1, w + 16)]
    return var[:max(5, n)]


class Case:
    """collects the planes of one case; make_specs() builds them afresh (same samples) for each of the two runs"""

    def __init__(self, layout, seed=0):
        self.layout, self.seed, self.items = layout, seed, []

    def add(self, name, role, dtype, h, w, data=None, poison_rows=()):
        self.items.append(dict(name=name, role=role, dtype=np.dtype(dtype), h=h, w=w, data=data, poison_rows=tuple(poison_rows)))
        return name

    def _spec(self, it, k):
        name, role, dtype, h, w, data = it["name"], it["role"], it["dtype"], it["h"], it["w"], it["data"]
        isz = dtype.itemsize
        kw = dict(data=data, poison_rows=it["poison_rows"])
        if self.layout == "tight_odd":
            return G.PlaneSpec(name, role, h, w, dtype, w, 0, **kw)
        if self.layout == "shift1":
            return G.PlaneSpec(name, role, h, w, dtype, _up(w, 32), isz, **kw)  # pitch 16-byte aligned, base one sample off
        if self.layout == "window":
            y0, x0 = 4, 7
            H, W = h + y0 + 5, w + x0 + 6
            if dtype == np.uint32:
                nb = fx.splitmix64_plane(1000 + 17 * k + self.seed, (H, W), np.uint16).astype(np.uint32) * np.uint32(65537)
            else:
                nb = fx.splitmix64_plane(1000 + 17 * k + self.seed, (H, W), dtype)  # live samples: full range integers, [0, 1) floats
            if role != "out":
                nb[y0:y0 + h, x0:x0 + w] = data
            return G.PlaneSpec(name, role, h, w, dtype, _up(W, 32), 0, window=(H, W, y0, x0), neighbours=nb, **kw)
        return G.PlaneSpec(name, role, h, w, dtype, _up(w, 32), 0, **kw)  # aligned16, odd_pad32, packed

    def make_specs(self):
        specs = [self._spec(it, k) for k, it in enumerate(self.items)]
        if self.layout == "packed":
            order = np.random.default_rng(self.seed + 5).permutation(len(specs))
            specs = [specs[i] for i in order]
        return specs

    def run(self, dev, call, expect, check_scalars=None):
        """call(P) with P[name] = DevPlane view of the arena"""
        def do(arena):
            P = {s.name: dev.wrap(arena.address(s.name), s.h, s.w, s.pitch, s.dtype) for s in arena.specs}
            out = call(P)
            dev.sync()
            return out
        return G.run_case(lambda: G.DeviceBackend(dev), self.make_specs, do, expect, check_scalars=check_scalars)


def content(seed, h, w, dtype, natural=False):
    a = fx.tiled_natural((h, w), dtype, seed % 3) if natural else fx.splitmix64_plane(seed, (h, w), dtype)
    return np.ascontiguousarray(a)


def in_out(layout, dtype, sizes, seed=0, natural=False):
    """src_i / dst_i for a plane table"""
    c = Case(layout, seed)
    datas = []
    for i, (h, w) in enumerate(sizes):
        a = content(seed + i, h, w, dtype, natural and i % 2 == 0)
        datas.append(a)
        c.add(f"src{i}", "in", dtype, h, w, a)
        c.add(f"dst{i}", "out", dtype, h, w)
    return c, datas


# ---------------------------------------------------------------------------------------------------------------
# Positive controls on the device: the arena must see what a real kernel does one sample too far. Both stay inside memory the case owns
# (the plane's own pitch padding: pitch 224 for w = 203).
def test_control_a_kernel_told_w_plus_1_is_caught_writing_the_padding(dev, oracle):
    c, (a,) = in_out("odd_pad32", np.uint8, [(37, 203)], seed=1)

    def call(P):
        wider = lambda p: dev.wrap(p.ptr, p.h, p.w + 1, p.stride, p.dtype)
        dev.limiter([wider(P["src0"])], [wider(P["dst0"])], [30.0], [200.0])
    with pytest.raises(G.FootprintError, match=r"plane 'dst0'.*write outside \[0, w\) x h: first at row 0, column 203 .*; 37 bytes differ \(poison 0x00"):
        c.run(dev, call, {"dst0": oracle.limiter(a, 30.0, 200.0)})


def test_control_a_reader_told_w_plus_1_is_caught_depending_on_the_padding(dev, oracle):
    c, (a,), _ = _reader_planes("odd_pad32", np.uint16, False, 21)
    one = [c.items[0]]
    c.items = one

    def call(P):
        p = P["src0"]
        return dev.plane_average([dev.wrap(p.ptr, p.h, p.w + 1, p.stride, p.dtype)])[0]
    with pytest.raises(G.FootprintError, match="scalars depend on bytes outside"):
        c.run(dev, call, {})


# ---------------------------------------------------------------------------------------------------------------
# BoxBlur. Which kernel a shape reaches (boxblur.hip, boxblur_ct.hpp:ring_ok / ring16_ok / run_ct_ring, boxblur_ctf.hip:ring_interior,
# boxblur_rt.hip:run_rt) — aligned16 / odd_pad32 / packed have 16-byte aligned bases and pitches, the other layouts do not:
#   ring kernel (CT integer, h >= 53, pitch >= 24): aligned16 -> the fast instance alone; odd_pad32 / packed -> fast tiles + the GENERAL
#   instance for the last tile(s) (w % 8 != 0); tight_odd / shift1 / window -> ring_ok is false (base or pitch & 15) -> launch_ct_int, the generic kernel.
BOXBLUR = {
    # name: (dtype, (h, w), (hr, hp, vr, vp), options, what it reaches)
    "ct_ring_u8_px16": (np.uint8, (72, 170), (5, 1, 5, 1), {}, "u8 ring kernel, 16 pixels a lane (w >= 32, r < 8: ring16_ok)"),
    "ct_ring_u8_px8": (np.uint8, (72, 170), (13, 1, 13, 1), {"VSZIP_CT_U8_PX8": 1}, "u8 ring kernel, 8 pixels a lane"),
    "ct_ring_u16": (np.uint16, (72, 170), (13, 1, 13, 1), {}, "u16 ring kernel (h >= 53, pitch >= 24)"),
    "ct_ring_u16_r22": (np.uint16, (60, 90), (22, 1, 22, 1), {}, "u16 ring kernel, largest radius, one band"),
    "ct_general_small": (np.uint8, (20, 37), (3, 1, 3, 1), {}, "h < 53: launch_ct_int"),
    "ct_general_scan1": (np.uint16, (72, 170), (7, 1, 7, 1), {"VSZIP_SCAN_MODE": 1}, "generic kernel + shuffle scan"),
    "ct_general_scan2": (np.uint8, (72, 170), (7, 1, 7, 1), {"VSZIP_SCAN_MODE": 2}, "generic kernel + DPP scan"),
    "ct_h_only_ring": (np.uint8, (72, 170), (7, 1, 0, 0), {}, "horizontal-only r <= 22: ring kernel with a one-row window (run_h)"),
    "ctf_f32": (np.float32, (96, 330), (5, 1, 5, 1), {}, "float ring interior + tile borders (ring_interior) or, unaligned, the tile kernel alone"),
    "ctf_f16": (np.float16, (96, 330), (5, 1, 5, 1), {}, "f16: the same split"),
    "ctf_f32_small": (np.float32, (11, 23), (2, 1, 2, 1), {}, "too small for the ring: tile kernel"),
    "rt_hsmall": (np.uint16, (40, 170), (3, 3, 0, 0), {}, "hsmall: r <= 16, >= 2 horizontal passes, integer"),
    "rt_hsmall_u8_r13": (np.uint8, (40, 170), (13, 2, 0, 0), {}, "hsmall with two neighbour groups a side"),
    "rt_ichain": (np.uint16, (200, 70), (0, 0, 5, 3), {"VSZIP_RT_ICHAIN_ALL": 1}, "integer vertical pass chain in bands"),
    "rt_ichain_whole": (np.uint8, (200, 70), (0, 0, 2, 5), {"VSZIP_RT_ICHAIN_ALL": 1, "VSZIP_RT_NO_BANDED": 1}, "integer vertical pass chain, whole columns"),
    "rt_fchain_v": (np.float32, (120, 170), (0, 0, 4, 3), {"VSZIP_RT_FCHAIN_ALL": 1}, "float pass chain, vertical"),
    "rt_fchain_h": (np.float16, (60, 170), (4, 3, 0, 0), {"VSZIP_RT_FCHAIN_ALL": 1}, "float pass chain, horizontal"),
    "rt_vband_hring": (np.uint8, (120, 170), (40, 1, 40, 1), {}, "radius above the CT limit: horizontal ring row kernel + vertical bands"),
    "rt_multi_both": (np.float32, (120, 170), (23, 2, 25, 2), {}, "several passes both ways, r > 22"),
    "rt_v_only": (np.uint16, (120, 170), (0, 0, 30, 1), {}, "vertical-only"),
    "rt_h_only_f32": (np.float32, (40, 170), (30, 1, 0, 0), {}, "horizontal-only float row kernel"),
    "rt_mixed_radii": (np.uint8, (97, 131), (4, 1, 9, 1), {}, "hradius != vradius: one RT pass each way"),
    # larger planes: several row bands and column tiles a plane, so band seams and the fast / GENERAL tile split lie inside the picture
    "ct_ring_u16_bands": (np.uint16, (400, 1000), (13, 1, 13, 1), {}, "u16 ring kernel, several bands and tiles"),
    "ct_ring_u8_px16_wide": (np.uint8, (300, 1100), (3, 1, 3, 1), {}, "u8 ring kernel, 16 pixels a lane, two tiles"),
    "ct_ring_u8_r22": (np.uint8, (300, 1100), (22, 1, 22, 1), {}, "u8 ring kernel, r > kRing16MaxR: 8 pixels a lane"),
    "ctf_f32_big": (np.float32, (200, 700), (13, 1, 13, 1), {}, "float ring interior with tile borders on all four sides"),
    "ctf_f16_big": (np.float16, (200, 700), (8, 1, 8, 1), {}, "f16 ring interior"),
    "rt_ichain_auto": (np.uint16, (540, 64), (0, 0, 13, 5), {}, "the integer chain as the library itself plans it (bands, split chains)"),
    "rt_gauss_u8": (np.uint8, (270, 480), (2, 3, 2, 3), {}, "hsmall + vertical chain, the Gaussian approximation scripts use"),
}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(BOXBLUR))
def test_boxblur(dev, oracle, name, layout):
    dtype, (h, w), args, opts, _ = BOXBLUR[name]
    mh, mw = 2 * args[2] + 1, 2 * args[0] + 1
    c, datas = in_out(layout, dtype, sizes_for(layout, h, w, 1, mh, mw), seed=len(name), natural=True)
    n = len(datas)

    def call(P):
        with dev.options(**opts):
            dev.boxblur([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], *args)
    c.run(dev, call, {f"dst{i}": oracle.boxblur(a, *args) for i, a in enumerate(datas)})


@pytest.mark.parametrize("layout", ["aligned16", "shift1"])
def test_boxblur_long_rows_need_alignment_or_are_refused(dev, oracle, layout):
    """the one alignment the header says is refused, not served: the RT integer row pass over rows longer than 16000 samples (boxblur_rt.hip:
    the scalar row kernel keeps a row's prefix in LDS). Aligned, the same rows are blurred; unaligned, VSZIP_ERR_UNSUPPORTED and nothing is touched."""
    h, w = 3, 16400 if layout == "shift1" else 16384
    src = content(5, h, w, np.uint8)
    c = Case(layout, 13)
    c.add("src0", "in", np.uint8, h, w, src)
    if layout == "aligned16":
        c.add("dst0", "out", np.uint8, h, w)
        c.run(dev, lambda P: dev.boxblur([P["src0"]], [P["dst0"]], 30, 1, 0, 0), {"dst0": oracle.boxblur(src, 30, 1, 0, 0)})
        return
    c.add("dst0", "in", np.uint8, h, w, content(6, h, w, np.uint8))

    def call(P):
        with pytest.raises(VszipError) as e:
            dev.boxblur([P["src0"]], [P["dst0"]], 30, 1, 0, 0)
        assert e.value.code == ERR_UNSUPPORTED, e.value
    c.run(dev, call, {})


# ---------------------------------------------------------------------------------------------------------------
BILATERAL = {
    # name: (dtype, sigmaS, sigmaR, kwargs, with ref)
    "tiled_u8": (np.uint8, 2, 2, dict(algorithm=[2]), False),               # radius 3 step 2 (walk kernel where tiled and not joint)
    "tiled_u16_walk36": (np.uint16, 3, 0.02, dict(algorithm=[2]), False),   # sigmaS = 3: radius 5 step 2, bilateral_walk36_kernel
    "tiled_f32_small_sigma": (np.float32, 0.8, 0.05, dict(algorithm=[2]), False),
    "tiled_f16": (np.float16, 5, 2, dict(algorithm=[2]), False),            # f16 never walks: the truncated-window tile kernel
    "tiled_u16_ref": (np.uint16, 3, 0.02, dict(algorithm=[2]), True),       # joint: no walk kernel, tile kernel with a ref plane
    "tiled_u8_ref": (np.uint8, 2, 2, dict(algorithm=[2]), True),
    "pbfic_u16": (np.uint16, 3, 0.1, dict(algorithm=[1], pbficnum=[4]), False),
    "pbfic_f32_ref": (np.float32, 3, 0.1, dict(algorithm=[1], pbficnum=[7]), True),
    "pbfic_u8": (np.uint8, 8, 2, dict(algorithm=[1], pbficnum=[0]), False),
}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(BILATERAL))
def test_bilateral(dev, oracle, name, layout):
    dtype, sS, sR, kw, with_ref = BILATERAL[name]
    dt = np.dtype(dtype)
    hist = (1 << (8 * dt.itemsize)) if dt.kind == "u" else 65536
    c, datas = in_out(layout, dtype, sizes_for(layout, 67, 131), seed=3, natural=True)
    n = len(datas)
    refs = None
    if with_ref:
        refs = [content(40 + i, a.shape[0], a.shape[1], dtype, True) for i, a in enumerate(datas)]
        for i, r in enumerate(refs):
            c.add(f"ref{i}", "in", dtype, r.shape[0], r.shape[1], r)
    cfg = dev.bilateral_cfg([sS], [sR], hist_len=hist, **kw)
    try:
        k = cfg[0]
        want = {f"dst{i}": oracle.bilateral_plane(a, k.sigmaS, k.sigmaR, k.algorithm, k.radius, k.step, k.pbficnum, ref=refs[i] if refs else None) for i, a in enumerate(datas)}

        def call(P):
            dev.bilateral([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], cfg, [0] * n, [P[f"ref{i}"] for i in range(n)] if refs else None)
        c.run(dev, call, want)
    finally:
        dev.bilateral_free(cfg)


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.float16, np.float32], ids=["u8", "u16", "u32", "f16", "f32"])
def test_limiter(dev, oracle, dtype, layout):
    dt = np.dtype(dtype)
    sizes = sizes_for(layout, 37, 203)
    if dt == np.uint32:
        c = Case(layout, 1)
        datas = []
        for i, (h, w) in enumerate(sizes):
            a = (fx.splitmix64_plane(i, (h, w), np.uint16).astype(np.uint32) << 16) | fx.splitmix64_plane(50 + i, (h, w), np.uint16)
            datas.append(a)
            c.add(f"src{i}", "in", dt, h, w, a)
            c.add(f"dst{i}", "out", dt, h, w)
        lo, hi = float(1 << 20), float(3 << 30)
        want = [np.clip(a, np.uint32(1 << 20), np.uint32(3 << 30)) for a in datas]  # the operation itself, in the sample type
    else:
        c, datas = in_out(layout, dtype, sizes, seed=1)
        lo, hi = (0.1, 0.8) if dt.kind == "f" else (float(np.iinfo(dt).max // 10), float(np.iinfo(dt).max // 10 * 8))
        want = [oracle.limiter(a, lo, hi) for a in datas]
    n = len(datas)

    def call(P):
        dev.limiter([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], [lo] * n, [hi] * n)
    c.run(dev, call, {f"dst{i}": w for i, w in enumerate(want)})


@pytest.mark.parametrize("filt", ["limiter_u8", "limit_filter_u16", "boxblur_ct_u16", "boxblur_ring_u8", "clahe_u8", "plane_average_u16"])
def test_tables_longer_than_one_launch(dev, oracle, filt):
    """more planes than one launch's table holds (192: limiter.hip kMaxPlanesL and its kin), of differing sizes, packed back to back in shuffled
    order: the per-plane block offsets (`block0` searches) and the split over launches, with every neighbour's guard watching"""
    import clahe_ref as cr

    ring = filt == "boxblur_ring_u8"
    n = 200 if not ring else 40
    dtype = np.uint8 if filt.endswith("u8") else np.uint16
    sizes = [((53 + i % 5) if ring else (9 + i % 11), (40 + 3 * (i % 13)) if ring else (17 + i % 37)) for i in range(n)]
    reader = filt.startswith("plane_average")
    c = Case("packed", 17)
    datas = []
    for i, (h, w) in enumerate(sizes):
        datas.append(content(i, h, w, dtype, i % 4 == 0))
        c.add(f"src{i}", "in", dtype, h, w, datas[i])
        if not reader:
            c.add(f"dst{i}", "out", dtype, h, w)
    S, D = (lambda P: [P[f"src{i}"] for i in range(n)]), (lambda P: [P[f"dst{i}"] for i in range(n)])
    check = None
    if filt == "limiter_u8":
        call, want = (lambda P: dev.limiter(S(P), D(P), [30.0] * n, [200.0] * n)), [oracle.limiter(a, 30.0, 200.0) for a in datas]
    elif filt == "limit_filter_u16":
        flt = [oracle.boxblur(a, 1, 1, 1, 1) for a in datas]
        call, want = (lambda P: dev.limit_filter(S(P), S(P), D(P), [2048.0] * n, [1024.0] * n, [2.0] * n)), [oracle.limit_filter(a, a, None, 2048.0, 1024.0, 2.0) for a in datas]
    elif filt.startswith("boxblur"):
        r = 2
        call, want = (lambda P: dev.boxblur(S(P), D(P), r, 1, r, 1)), [oracle.boxblur(a, r, 1, r, 1) for a in datas]
    elif filt == "clahe_u8":
        call, want = (lambda P: dev.clahe(S(P), D(P), 4, 3)), [cr.clahe(a, 4, (3, 3)) for a in datas]
    else:
        want = []
        call = lambda P: dev.plane_average(S(P))[0]

        def check(v):
            for i, a in enumerate(datas):
                assert v[i] == pytest.approx(oracle.plane_average(a)[0], rel=1e-12), i
    c.run(dev, call, {f"dst{i}": w for i, w in enumerate(want)}, check)


def _inplace_case(layout, dtype, sizes, seed):
    c = Case(layout, seed)
    datas = []
    for i, (h, w) in enumerate(sizes):
        a = content(seed + i, h, w, dtype, i % 2 == 0)
        datas.append(a)
        c.add(f"p{i}", "inout", dtype, h, w, a)
    return c, datas


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("with_refs", [False, True], ids=["src", "refs"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float16], ids=["u8", "u16", "f32", "f16"])
def test_limit_filter(dev, oracle, dtype, with_refs, layout):
    dt = np.dtype(dtype)
    is_f = dt.kind == "f"
    c = Case(layout, 2)
    sizes = sizes_for(layout, 45, 203, 1, 9, 9)
    srcs, flts, refs = [], [], []
    for i, (h, w) in enumerate(sizes):
        s = content(i, h, w, dtype, True)
        srcs.append(s)
        flts.append(oracle.boxblur(s, 2, 1, 2, 1))
        refs.append(oracle.boxblur(s, 4, 1, 4, 1) if with_refs else None)
        c.add(f"flt{i}", "in", dtype, h, w, flts[i])
        c.add(f"src{i}", "in", dtype, h, w, s)
        if with_refs:
            c.add(f"ref{i}", "in", dtype, h, w, refs[i])
        c.add(f"dst{i}", "out", dtype, h, w)
    n = len(sizes)
    bits = 32 if is_f else 8 * dt.itemsize
    dark = oracle.scale_value_from_8bit(8, is_f, bits, False)
    bright = oracle.scale_value_from_8bit(4, is_f, bits, not is_f)

    def call(P):
        g = lambda r: [P[f"{r}{i}"] for i in range(n)]
        dev.limit_filter(g("flt"), g("src"), g("dst"), [dark] * n, [bright] * n, [2.0] * n, g("ref") if with_refs else None)
    c.run(dev, call, {f"dst{i}": oracle.limit_filter(flts[i], srcs[i], refs[i], dark, bright, 2.0) for i in range(n)})


@pytest.mark.parametrize("layout", LAYOUTS)
def test_adaptive_binarize(dev, oracle, layout):
    c = Case(layout, 4)
    sizes = sizes_for(layout, 45, 203, 1, 9, 9)
    a, b = [], []
    for i, (h, w) in enumerate(sizes):
        a.append(content(i, h, w, np.uint8, True))
        b.append(oracle.boxblur(a[i], 3, 1, 3, 1))
        c.add(f"clip{i}", "in", np.uint8, h, w, a[i])
        c.add(f"blur{i}", "in", np.uint8, h, w, b[i])
        c.add(f"dst{i}", "out", np.uint8, h, w)
    n = len(sizes)

    def call(P):
        g = lambda r: [P[f"{r}{i}"] for i in range(n)]
        dev.adaptive_binarize(g("clip"), g("blur"), g("dst"), 3)
    c.run(dev, call, {f"dst{i}": oracle.adaptive_binarize(a[i], b[i], 3) for i in range(n)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("filt", ["limiter_u16", "limiter_f32", "limit_filter_u8", "limit_filter_dst_is_src", "adaptive_binarize", "adaptive_binarize_dst_is_clip2", "clahe_u8", "clahe_u16"])
def test_in_place(dev, oracle, filt, layout):
    """dst == src, which the header allows for the point filters and CLAHE: the plane comes back as the oracle's output, nothing around it changes"""
    import clahe_ref as cr

    dtype = {"limiter_u16": np.uint16, "limiter_f32": np.float32, "clahe_u16": np.uint16}.get(filt, np.uint8)
    c, datas = _inplace_case(layout, dtype, sizes_for(layout, 45, 203, 1, 9, 9), 6)
    n = len(datas)
    g = lambda P: [P[f"p{i}"] for i in range(n)]
    if filt.startswith("limiter"):
        lo, hi = (0.2, 0.7) if filt.endswith("f32") else (9000.0, 40000.0)
        call = lambda P: dev.limiter(g(P), g(P), [lo] * n, [hi] * n)
        want = [oracle.limiter(a, lo, hi) for a in datas]
    elif filt == "limit_filter_u8":  # dst == flt, the source clip separate
        srcs = [content(70 + i, a.shape[0], a.shape[1], dtype, True) for i, a in enumerate(datas)]
        for i, s in enumerate(srcs):
            c.add(f"src{i}", "in", dtype, s.shape[0], s.shape[1], s)
        call = lambda P: dev.limit_filter(g(P), [P[f"src{i}"] for i in range(n)], g(P), [8.0] * n, [4.0] * n, [2.0] * n)
        want = [oracle.limit_filter(a, s, None, 8.0, 4.0, 2.0) for a, s in zip(datas, srcs)]
    elif filt == "limit_filter_dst_is_src":  # dst == the source clip's plane (planes[i].ref), the filtered clip separate
        flts = [oracle.boxblur(a, 2, 1, 2, 1) for a in datas]
        for i, f in enumerate(flts):
            c.add(f"flt{i}", "in", dtype, f.shape[0], f.shape[1], f)
        call = lambda P: dev.limit_filter([P[f"flt{i}"] for i in range(n)], g(P), g(P), [8.0] * n, [4.0] * n, [2.0] * n)
        want = [oracle.limit_filter(f, a, None, 8.0, 4.0, 2.0) for f, a in zip(flts, datas)]
    elif filt == "adaptive_binarize_dst_is_clip2":
        clips = [content(80 + i, a.shape[0], a.shape[1], dtype, True) for i, a in enumerate(datas)]
        for i, s_ in enumerate(clips):
            c.add(f"clip{i}", "in", dtype, s_.shape[0], s_.shape[1], s_)
        call = lambda P: dev.adaptive_binarize([P[f"clip{i}"] for i in range(n)], g(P), g(P), 3)
        want = [oracle.adaptive_binarize(k, a, 3) for k, a in zip(clips, datas)]
    elif filt == "adaptive_binarize":  # dst == clip
        blur = [oracle.boxblur(a, 3, 1, 3, 1) for a in datas]
        for i, s in enumerate(blur):
            c.add(f"blur{i}", "in", dtype, s.shape[0], s.shape[1], s)
        call = lambda P: dev.adaptive_binarize(g(P), [P[f"blur{i}"] for i in range(n)], g(P), 3)
        want = [oracle.adaptive_binarize(a, b, 3) for a, b in zip(datas, blur)]
    else:
        call = lambda P: dev.clahe(g(P), g(P), 7, [3, 2])
        want = [cr.clahe(a, 7, (3, 2)) for a in datas]
    c.run(dev, call, {f"p{i}": w for i, w in enumerate(want)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tiles", [(3, 3), (8, 2)], ids=["3x3", "8x2"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_clahe(dev, dtype, tiles, layout):
    import clahe_ref as cr

    c, datas = in_out(layout, dtype, sizes_for(layout, 101, 257, 1, 16, 16), seed=8, natural=True)
    n = len(datas)

    def call(P):
        dev.clahe([P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], 7, list(tiles))
    c.run(dev, call, {f"dst{i}": cr.clahe(a, 7, tiles) for i, a in enumerate(datas)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_chain_run(dev, oracle, dtype, layout):
    """a two-stage chain (BoxBlur, then Limiter) with the intermediate plane owned by the context"""
    dt = np.dtype(dtype)
    c, datas = in_out(layout, dtype, sizes_for(layout, 72, 170, 1, 9, 9), seed=9, natural=True)
    n = len(datas)
    lo, hi = (0.2, 0.7) if dt.kind == "f" else (float(np.iinfo(dt).max // 5), float(np.iinfo(dt).max // 5 * 3))
    stages = [{"boxblur": (3, 1, 3, 1)}, {"limiter": ([lo] * 3, [hi] * 3)}]

    def call(P):
        dev.chain_run(stages, [P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], [i % 3 for i in range(n)])
    c.run(dev, call, {f"dst{i}": oracle.limiter(oracle.boxblur(a, 3, 1, 3, 1), lo, hi) for i, a in enumerate(datas)})


# ---------------------------------------------------------------------------------------------------------------
# EEDI3 (eedi3.hip: `general` = hp || mdis > kMaxMdis; lines of <= 1024 samples take one column a thread, the chain the chroma of a 1080p frame takes).
EEDI3 = {
    "tuned_f1": dict(field=1), "tuned_f0": dict(field=0), "tuned_dh_f1": dict(field=1, dh=True), "tuned_dh_f0": dict(field=0, dh=True),
    "tuned_vcheck0": dict(field=1, vcheck=0), "tuned_dh_vcheck0": dict(field=0, dh=True, vcheck=0), "masked_mdis8": dict(field=1, mdis=8, nrad=3),
    "general_hp": dict(field=1, hp=True), "general_hp_dh": dict(field=0, hp=True, dh=True), "general_mdis40": dict(field=1, mdis=40, nrad=3, vcheck=0),
    "sclip": dict(field=1, sclip=True), "sclip_dh": dict(field=0, dh=True, sclip=True), "mclip": dict(field=1, mclip=True), "mclip_dh_hp": dict(field=0, dh=True, hp=True, mclip=True),
    "wide_two_columns": dict(field=1, size=(16, 1100)), "wide_dh_sclip": dict(field=0, dh=True, sclip=True, size=(16, 2100)),  # lines > 1024 / > 2048 samples: 2 / 3 columns a thread
    "h_f1": dict(field=1, horizontal=True), "h_dh": dict(field=0, dh=True, horizontal=True), "h_sclip_vcheck0": dict(field=1, horizontal=True, sclip=True, vcheck=0),
}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(EEDI3))
def test_eedi3(dev, oracle, name, layout):
    """With dh = 0 the source rows of parity `field` are not inputs: they are interpolated. The vertical form uploads poison there instead of
    picture content, so a kernel that read one would differ between the two runs (and from the oracle under 0xFF)."""
    kw = dict(EEDI3[name])
    field, dh, hz = kw.pop("field"), kw.get("dh", False), kw.get("horizontal", False)
    with_s, with_m = kw.pop("sclip", False), kw.pop("mclip", False)
    bh, bw = kw.pop("size", (48, 140))
    c = Case(layout, 11)
    sizes = sizes_for(layout, bh, bw) if layout != "packed" else [(bh, bw), (bh - 8, bw + 9), (bh // 2 + 2, bw - 49), (bh + 4, bw - 5), (bh // 2, bw - 50)]
    if hz and not dh and layout == "packed":
        sizes = [(h, w + (w & 1)) for h, w in sizes]
    # createImpl's check, mirrored by the entry point: without dh the interpolated axis must be mod 2. EEDI3H on the odd-width layouts is refused.
    refused = hz and not dh and any(w & 1 for _, w in sizes)
    want, n = {}, len(sizes)
    for i, (h, w) in enumerate(sizes):
        src = content(i, h, w, np.float32, True)
        oh, ow = (h, w * (2 if dh else 1)) if hz else (h * (2 if dh else 1), w)
        sc = content(30 + i, oh, ow, np.float32) if with_s else None
        mc = (content(60 + i, h, w, np.uint8) > 128).astype(np.uint8) * 255 if with_m else None
        dead = () if (dh or hz) else tuple(range(field, h, 2))
        c.add(f"src{i}", "in", np.float32, h, w, src, poison_rows=dead)
        if with_s:
            c.add(f"sclip{i}", "in", np.float32, oh, ow, sc)
        if with_m:
            c.add(f"mclip{i}", "in", np.uint8, h, w, mc)
        if refused:
            c.add(f"dst{i}", "in", np.float32, oh, ow, content(90 + i, oh, ow, np.float32))  # a refused call writes nothing: the plane comes back as it was
            continue
        c.add(f"dst{i}", "out", np.float32, oh, ow)
        osrc = src.copy()
        for r in dead:
            osrc[r] = np.float32(-7.0)  # whatever these rows hold must not matter to the oracle either
        want[f"dst{i}"] = oracle.eedi3(osrc, field, sclip=sc, mclip=mc, **kw)

    def call(P):
        g = lambda r: [P[f"{r}{i}"] for i in range(n)]
        run = lambda: dev.eedi3_into(g("src"), g("dst"), field, sclips=g("sclip") if with_s else None, mclips=g("mclip") if with_m else None, **kw)
        if not refused:
            return run()
        with pytest.raises(VszipError) as e:
            run()
        assert e.value.code == ERR_ARG, e.value
    c.run(dev, call, want)


# ---------------------------------------------------------------------------------------------------------------
# Readers: inputs and guards untouched, the same scalars under both poisons, equal to the oracle.
def _reader_planes(layout, dtype, with_ref, seed, h=67, w=211):
    c = Case(layout, seed)
    a, b = [], []
    for i, (hh, ww) in enumerate(sizes_for(layout, h, w)):
        a.append(content(seed + i, hh, ww, dtype, i % 2 == 0))
        c.add(f"src{i}", "in", dtype, hh, ww, a[i])
        if with_ref:
            b.append(content(seed + 20 + i, hh, ww, dtype, i % 2 == 1))
            c.add(f"ref{i}", "in", dtype, hh, ww, b[i])
    return c, a, (b if with_ref else None)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("with_ref", [False, True], ids=["", "clipb"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16, np.float32], ids=["u8", "u16", "f16", "f32"])
def test_plane_average(dev, oracle, dtype, with_ref, layout):
    c, a, b = _reader_planes(layout, dtype, with_ref, 21)
    n = len(a)
    ex = (0, 255) if np.dtype(dtype).kind == "u" else ()

    def call(P):
        avg, diff = dev.plane_average([P[f"src{i}"] for i in range(n)], ex, [P[f"ref{i}"] for i in range(n)] if with_ref else None)
        return avg + (diff or [])

    def check(v):
        for i in range(n):
            oa, od = oracle.plane_average(a[i], ex, b[i] if with_ref else None)
            assert v[i] == pytest.approx(oa, rel=1e-12), (i, v[i], oa)
            if with_ref:
                assert v[n + i] == pytest.approx(od, rel=1e-12), (i, v[n + i], od)
    c.run(dev, call, {}, check)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("thr", [(0.0, 0.0), (0.05, 0.1)], ids=["exact", "thr"])
@pytest.mark.parametrize("with_ref", [False, True], ids=["", "clipb"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_plane_minmax(dev, oracle, dtype, with_ref, thr, layout):
    """two calls in a row: the second takes the sweep that the first call's result predicts (16-bit / float planes with thresholds)"""
    c, a, b = _reader_planes(layout, dtype, with_ref, 23)
    n = len(a)

    def call(P):
        out = []
        for _ in range(2):
            mn, mx, df = dev.plane_minmax([P[f"src{i}"] for i in range(n)], thr[0], thr[1], [P[f"ref{i}"] for i in range(n)] if with_ref else None)
            out += mn + mx + (df or [])
        return out

    def check(v):
        per = n * (3 if with_ref else 2)
        for rep in range(2):
            r = v[rep * per:(rep + 1) * per]
            for i in range(n):
                omn, omx, odf = oracle.plane_minmax(a[i], thr[0], thr[1], b[i] if with_ref else None)
                assert (r[i], r[n + i]) == (omn, omx), (rep, i)
                if with_ref:
                    assert r[2 * n + i] == (odf if np.dtype(dtype).kind == "u" else pytest.approx(odf, rel=1e-12)), (rep, i)
    c.run(dev, call, {}, check)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype,depth", [(np.uint8, 8), (np.uint16, 10)], ids=["u8", "u16_10"])
def test_xpsnr_wsse_batch(dev, oracle, dtype, depth, layout):
    """even widths and heights take the strip kernels, odd ones (and widths 2 mod 4 on a tight pitch) the per-block kernels (xpsnr.hip: `strips`); three frames, so that the temporal
    terms read both previous lumas. Every frame shares the geometry and the pitches, as the entry point requires."""
    h = 96
    if layout == "aligned16":
        wy, wc = 192, 96
    elif layout == "packed":
        wy, wc = 200, 100  # frames packed back to back: 3 frames x (3 org + 3 rec) planes of two sizes
    else:
        wy, wc, h = 202, 101, 94  # a 4:2:0 clip has no odd luma: odd chroma (47 x 101, the per-block kernels) under a luma that is 2 mod 4
    hc = h // 2
    peak = (1 << depth) - 1
    rng = np.random.default_rng(31)
    c = Case(layout, 31)
    orgs, recs = [], []
    for f in range(3):
        o = [rng.integers(0, peak + 1, s).astype(dtype) for s in ((h, wy), (hc, wc), (hc, wc))]
        r = [np.clip(p.astype(np.int64) + rng.integers(-9, 10, p.shape), 0, peak).astype(dtype) for p in o]
        orgs.append(o)
        recs.append(r)
        for k in range(3):
            c.add(f"org{f}_{k}", "in", dtype, o[k].shape[0], o[k].shape[1], o[k])
            c.add(f"rec{f}_{k}", "in", dtype, r[k].shape[0], r[k].shape[1], r[k])
    want = [oracle.xpsnr_wsse(orgs[f], recs[f], orgs[f - 1][0] if f > 0 else None, orgs[f - 2][0] if f > 1 else None, depth=depth, frame_rate=60) for f in range(3)]

    def call(P):
        O = [[P[f"org{f}_{k}"] for k in range(3)] for f in range(3)]
        R = [[P[f"rec{f}_{k}"] for k in range(3)] for f in range(3)]
        got = dev.xpsnr_wsse_batch(O, R, [None, O[0][0], O[1][0]], [None, None, O[0][0]], depth=depth, frame_rate=60)
        return [float(x) for fr in got for x in fr]  # (< 2^53: exact in a double)

    def check(v):
        assert v == [float(x) for fr in want for x in fr], (v, want)
    c.run(dev, call, {}, check)


SSIM_TOL = 1e-7  # tests/test_gpu_ssimulacra2.py, tests/test_gpu_ssim_yuv.py, tests/test_gpu_ssim_prestage.py


def _lin(v):
    v = v.astype(np.float64)
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4).astype(np.float32)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ssimulacra2(dev, oracle, layout):
    """linear RGBS planes, one pitch for all of them; packed: two pairs in one call, their twelve planes shuffled"""
    h, w = 70, lw(layout, 150)
    pairs = 2 if layout == "packed" else 1
    rng = np.random.default_rng(41)
    c = Case(layout, 41)
    R, D = [], []
    for p in range(pairs):
        ref = [_lin(np.roll(fx.tiled_natural((h, w), np.float32, k), 5 * p, axis=1)) for k in range(3)]
        dis = [np.clip(x + rng.normal(0, 0.03, x.shape).astype(np.float32), 0, 1).astype(np.float32) for x in ref]
        R.append(ref)
        D.append(dis)
        for k in range(3):
            c.add(f"ref{p}_{k}", "in", np.float32, h, w, ref[k])
            c.add(f"dis{p}_{k}", "in", np.float32, h, w, dis[k])
    want = [oracle.ssimulacra2(R[p], D[p]) for p in range(pairs)]

    def call(P):
        return dev.ssimulacra2([P[f"ref{p}_{k}"] for p in range(pairs) for k in range(3)], [P[f"dis{p}_{k}"] for p in range(pairs) for k in range(3)])

    def check(v):
        for g, e in zip(v, want):
            assert g == pytest.approx(e, abs=SSIM_TOL), (v, want)
    c.run(dev, call, {}, check)


SOURCES = {"RGB24": ("RGB", 8, 0, 0), "YUV420P8": ("YUV", 8, 1, 1), "YUV444P16": ("YUV", 16, 0, 0)}


def _source_clip(name, layout, shift=0):
    from oracle import vs_host as vh

    family, bits, ssw, ssh = SOURCES[name]
    h = 64
    w = lw(layout, 150, even=True) if layout != "packed" else 148
    rgb = np.ascontiguousarray(np.roll(fx.crop_rgb24()[:, 20:20 + h, 30:30 + w], shift, axis=2))
    if family == "RGB":
        return [np.ascontiguousarray(p) for p in rgb], rgb
    return [np.ascontiguousarray(p) for p in vh.rgb24_to_yuv(rgb, bits, ssw, ssh)], rgb


def _linear(name, planes):
    from oracle import vs_host as vh

    family, bits, ssw, ssh = SOURCES[name]
    return vh.to_linear_rgbs(planes, family, bits) if family == "RGB" else vh.yuv_to_linear_rgbs(planes, bits, ssw, ssh, 1, 0)


def _fmt(dev, name, planes):
    family, bits, ssw, ssh = SOURCES[name]
    return dev.ssim_source(family, planes[0].dtype, bits, True, ssw=ssw, ssh=ssh)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(SOURCES))
def test_to_rgbs_linear(dev, name, layout):
    """the pre-stage alone: three source planes in, three f32 planes out (bit-exact, as tests/test_gpu_ssim_prestage.py and test_gpu_ssim_yuv.py)"""
    planes, _ = _source_clip(name, layout)
    c = Case(layout, 43)
    for k, p in enumerate(planes):
        c.add(f"src{k}", "in", p.dtype, p.shape[0], p.shape[1], p)
    h, w = planes[0].shape
    for k in range(3):
        c.add(f"dst{k}", "out", np.float32, h, w)
    want = _linear(name, planes)

    def call(P):
        dev.to_rgbs_linear_into(_fmt(dev, name, planes), [P[f"src{k}"] for k in range(3)], [P[f"dst{k}"] for k in range(3)])
    c.run(dev, call, {f"dst{k}": np.ascontiguousarray(want[k], np.float32) for k in range(3)})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(SOURCES))
def test_ssimulacra2_src(dev, oracle, name, layout):
    from oracle import vs_host as vh

    pairs = 2 if layout == "packed" else 1
    c = Case(layout, 47)
    want = []
    for p in range(pairs):
        ref, _ = _source_clip(name, layout, shift=3 * p)
        dis = [vh.std_boxblur(x, 1, 1) for x in ref]
        for k in range(3):
            c.add(f"ref{p}_{k}", "in", ref[k].dtype, ref[k].shape[0], ref[k].shape[1], ref[k])
            c.add(f"dis{p}_{k}", "in", dis[k].dtype, dis[k].shape[0], dis[k].shape[1], np.ascontiguousarray(dis[k]))
        want.append(oracle.ssimulacra2(_linear(name, ref), _linear(name, dis)))
        first = ref

    def call(P):
        return dev.ssimulacra2_src(_fmt(dev, name, first), [P[f"ref{p}_{k}"] for p in range(pairs) for k in range(3)], [P[f"dis{p}_{k}"] for p in range(pairs) for k in range(3)])

    def check(v):
        for g, e in zip(v, want):
            assert g == pytest.approx(e, abs=SSIM_TOL), (v, want)
    c.run(dev, call, {}, check)
