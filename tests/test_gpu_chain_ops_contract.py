"""vszip_chain_ops, the rest of its contract (include/vszip_hip.h, rules 2, 4 and 5): a chain that is not well formed is refused before anything is
queued; a chain writes only [0, w) x h of the caller's dst planes and leaves src alone, in every layout of tests/test_gpu_footprint.py; and the
chain buffer may grow in the middle of a queue."""
import numpy as np
import pytest

import fixtures as fx
from test_gpu_footprint import LAYOUTS, in_out, sizes_for

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def same(got, want) -> bool:
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def table(dev, dtype, frames=2, shapes=((40, 64), (20, 32), (20, 32)), extra=None):
    """frames x 3 planes (and one plane of another size as a further luma frame: extra), the destinations filled with the sentinel"""
    host = [fx.splitmix64_plane(50 + 3 * f + k, s, dtype) for f in range(frames) for k, s in enumerate(shapes)]
    slots = [0, 1, 2] * frames
    nums = [f for f in range(frames) for _ in range(3)]
    if extra is not None:
        host.append(fx.splitmix64_plane(99, extra, dtype))
        slots.append(0)
        nums.append(frames)
    ds = [dev.upload(p) for p in host]
    dd = [dev.upload(np.full((p.shape[0], p.shape[1] * p.itemsize), SENTINEL, np.uint8).view(dtype)) for p in host]
    return host, ds, dd, slots, nums


def untouched(dev, dd):
    dev.sync()
    return all((dev.download(d).view(np.uint8) == SENTINEL).all() for d in dd)


BLUR = {"boxblur": (1, 1, 1, 1)}  # first in every refused chain: it would write the dst planes of slots 1 and 2 directly, were anything queued
LUMA = (True, False, False)


def refusals(tb):
    """(name, dtype, ops after BLUR, table changes, text) of every refusal of rule 4"""
    u8, u16, f32, f16 = np.uint8, np.uint16, np.float32, np.float16
    mosq = dict(strength=16)
    return [
        ("kind number", u8, [{"raw": (11, 1), "planes": LUMA}], {}, "op 1: kind 11"),
        ("negative kind", u8, [{"raw": (-1, 1), "planes": LUMA}], {}, "op 1: kind -1"),
        ("NULL params", u8, [{"raw": (6, None), "planes": LUMA}], {}, r"op 1 \(Checkmate\): params is NULL"),
        ("NULL params of an op that filters nothing", u16, [{"raw": (0, None), "planes": (False, False, False)}], {}, r"op 1 \(BoxBlur\): params is NULL"),
        ("Compress on u16", u16, [{"compress": tb, "planes": LUMA}], {}, r"op 1 \(Compress\) does not take sample type 1"),
        ("CombMaskMT on u16", u16, [{"comb_mask_mt": (30, 30), "planes": LUMA}], {}, r"op 1 \(CombMaskMT\) does not take sample type 1"),
        ("CombMask on u16", u16, [{"comb_mask": dict(mthresh=0), "planes": LUMA}], {}, r"op 1 \(CombMask\) does not take sample type 1"),
        ("Checkmate on u16", u16, [{"checkmate": {}, "planes": LUMA}], {}, r"op 1 \(Checkmate\) does not take sample type 1"),
        ("Checkmate on f32, as op 2", f32, [dict(BLUR), {"checkmate": {}, "planes": LUMA}], {}, r"op 2 \(Checkmate\) does not take sample type 3"),
        ("CLAHE on f32", f32, [{"clahe": (7, 3), "planes": LUMA}], {}, r"op 1 \(CLAHE\) does not take sample type 3"),
        ("Deband on u8", u8, [{"raw": (8, 1), "planes": LUMA}], {}, r"op 1 \(Deband\) does not take sample type 0"),
        ("MosquitoNR on f16", f16, [{"mosquito_nr": mosq, "planes": LUMA}], {}, r"op 1 \(MosquitoNR\) does not take sample type 2"),
        ("BilateralDither on f16", f16, [{"raw": (9, 1), "planes": LUMA}], {}, r"op 1 \(BilateralDither\) does not take sample type 2"),
        ("bits on u8", u8, [{"mosquito_nr": mosq, "planes": LUMA}], dict(bits=10), r"op 1 \(MosquitoNR\): bits_per_sample 10 does not fit sample type 0"),
        ("bits on u16", u16, [{"mosquito_nr": mosq, "planes": LUMA}], dict(bits=8), r"op 1 \(MosquitoNR\): bits_per_sample 8 does not fit sample type 1"),
        ("no frame numbers", u8, [{"checkmate": {}, "planes": LUMA}], dict(frames=None), r"op 1 \(Checkmate\) reads neighbouring frames: the table needs frame numbers"),
        ("no frame numbers, CombMask", u8, [{"comb_mask": dict(mthresh=9), "planes": LUMA}], dict(frames=None), r"op 1 \(CombMask\) reads neighbouring frames"),
        ("a gap in the frames", u8, [{"checkmate": {}, "planes": LUMA}], dict(frames=[0, 0, 0, 2, 2, 2]), "have a gap"),
        ("a gap in one slot", u8, [{"checkmate": {}, "planes": LUMA}], dict(frames=[0, 0, 0, 1, 1, 3]), "of slot 2 have a gap"),
        ("a (slot, frame) pair twice", u8, [{"checkmate": {}, "planes": LUMA}], dict(frames=[0, 0, 0, 0, 1, 1]), "plane 3 is frame 0 of slot 0 a second time"),
        ("mixed sizes in a slot", u8, [{"checkmate": {}, "planes": LUMA}], dict(extra=(24, 40)), "plane 6 differs in size from the other planes of slot 0"),
        ("slot 3", u8, [{"checkmate": {}, "planes": LUMA}], dict(slots=[0, 1, 2, 0, 1, 3]), "bad plane 5"),
        ("slot -1", u16, [dict(BLUR)], dict(slots=[0, -1, 2, 0, 1, 2]), "bad plane 1"),
        ("NULL strength", u8, [{"raw": (7, "zeros"), "planes": LUMA}], {}, r"op 1 \(MosquitoNR\): strength is NULL"),
        ("NULL per", u16, [{"raw": (8, "zeros"), "planes": LUMA}], {}, r"op 1 \(Deband\): per is NULL"),
        ("NULL tables", u8, [{"raw": (10, "zeros"), "planes": LUMA}], {}, r"op 1 \(Compress\): tables is NULL"),
    ]


def test_refusals_queue_nothing_and_the_next_call_is_right(dev):
    """every refusal of rule 4: VszipError (VSZIP_ERR_ARG) naming the op, and the dst planes, filled with a sentinel before, are as they were after a
    synchronise - the BoxBlur that comes first in each chain has not run. Then a valid chain on the same context is right."""
    import ctypes as C

    from vszip_amd import capi

    tb = capi.compress_tables()
    zeros = C.create_string_buffer(64)  # a params block of NULL pointers
    cases = refusals(tb)
    assert len(cases) >= 20
    for name, dtype, ops, change, text in cases:
        host, ds, dd, slots, nums = table(dev, dtype, extra=change.get("extra"))
        for op in ops:
            if "raw" in op:
                kind, prm = op["raw"]
                op["raw"] = (kind, C.addressof(zeros) if prm in (1, "zeros") else None)
        kw = dict(frames=change["frames"] if "frames" in change else nums, bits=change.get("bits"))
        with pytest.raises(capi.VszipError, match=text) as e:
            dev.chain_ops([dict(BLUR)] + ops, ds, dd, change.get("slots", slots), **kw)
        assert e.value.code == capi.ERR_ARG, name
        assert untouched(dev, dd), name
    # a value check stays with the entry point and keeps its wording; what dst holds then is unspecified
    host, ds, dd, slots, nums = table(dev, np.uint8)
    with pytest.raises(capi.VszipError, match=r"MosquitoNR: strength value 33 is above maximum 32\."):
        dev.chain_ops([dict(BLUR), {"mosquito_nr": dict(strength=33), "planes": LUMA}], ds, dd, slots)
    # ... and the context goes on: a valid temporal chain against its twin
    ops = [dict(BLUR), {"compress": tb, "chroma": [int(s > 0) for s in slots]}, {"checkmate": dict(tthr2=4)}]
    dev.chain_ops(ops, ds, dd, slots, frames=nums)
    a = [dev.empty(p.h, p.w, p.dtype) for p in ds]
    dev.boxblur(ds, a, 1, 1, 1, 1)
    b = [dev.empty(p.h, p.w, p.dtype) for p in ds]
    dev.compress(a, b, tb, [int(s > 0) for s in slots])
    c = [dev.empty(p.h, p.w, p.dtype) for p in ds]
    dev.checkmate_clip([b[:3], b[3:]], [c[:3], c[3:]], tthr2=4)
    for i in range(len(ds)):
        assert same(dev.download(dd[i]), dev.download(c[i])), i


@pytest.mark.parametrize("layout", LAYOUTS)
def test_footprint_of_a_mixed_chain(dev, layout):
    """BoxBlur -> MosquitoNR(slot 0) -> CLAHE(slot 0) -> Limiter(slots 1, 2) on u16 planes in the guarded arena: slot 0 has three writers and uses both
    halves of its region, slots 1 and 2 one half; the last writer of each entry stores into the caller's pitch and alignment. Expected samples: the same
    entry points one after another on ordinary planes (tests/test_gpu_chain_ops.py ties the two together; the entry points' own footprints are
    tests/test_gpu_footprint.py and its companions)."""
    c, datas = in_out(layout, np.uint16, sizes_for(layout, 72, 170, 1, 16, 16), seed=21, natural=True)
    n = len(datas)
    slots = [i % 3 for i in range(n)]
    lo, hi = [0.0, 9000.0, 9000.0], [65535.0, 50000.0, 50000.0]
    ops = [{"boxblur": (2, 1, 2, 1)}, {"mosquito_nr": dict(strength=20), "planes": LUMA}, {"clahe": (7, [3, 2]), "planes": LUMA}, {"limiter": (lo, hi), "planes": (False, True, True)}]
    want = []
    for a, s in zip(datas, slots):
        p, q = dev.upload(a), dev.empty(a.shape[0], a.shape[1], a.dtype)
        dev.boxblur([p], [q], 2, 1, 2, 1)
        if s == 0:
            dev.mosquito_nr([q], [p], strength=20, bits=16)
            dev.clahe([p], [q], 7, [3, 2])
        else:
            dev.limiter([q], [p], [lo[s]], [hi[s]])
        want.append(dev.download(q if s == 0 else p))
        assert not same(want[-1], a)

    def call(P):
        dev.chain_ops(ops, [P[f"src{i}"] for i in range(n)], [P[f"dst{i}"] for i in range(n)], slots, bits=16)
    c.run(dev, call, {f"dst{i}": w for i, w in enumerate(want)})


def test_chain_buffer_grows_mid_queue():
    """three vszip_chain_ops calls on one context with no host synchronise in between - u8 planes of 64 x 48, of 256 x 192, of 64 x 48 again, each with
    its own content; Compress -> MosquitoNR -> CombMaskMT on every plane, so each entry has three writers and uses both halves of its region.
    Expected: the same call made alone on a fresh context."""
    import vszip_amd
    from vszip_amd import capi

    tb = capi.compress_tables(codec=0, qscale=6)
    ops = [{"compress": tb, "chroma": [0, 1, 1]}, {"mosquito_nr": dict(strength=24)}, {"comb_mask_mt": (10, 40)}]
    calls = [[fx.tiled_natural(shape, np.uint8, i) // 2 + fx.splitmix64_plane(8000 + 10 * c + i, shape, np.uint8) // 8 for i in range(3)]
             for c, shape in enumerate([(48, 64), (192, 256), (48, 64)])]

    def run(d, calls):
        tables = [([d.upload(np.ascontiguousarray(p)) for p in planes], [d.empty(p.shape[0], p.shape[1], np.uint8) for p in planes]) for planes in calls]
        for srcs, dsts in tables:  # (uploads synchronise: all of them before the first call)
            d.chain_ops(ops, srcs, dsts, [0, 1, 2])
        return [[d.download(o) for o in dsts] for _, dsts in tables]

    d = vszip_amd.Device(0)
    try:
        got = run(d, calls)
    finally:
        d.close()
    for c, planes in enumerate(calls):
        alone = vszip_amd.Device(0)
        try:
            want = run(alone, [planes])[0]
        finally:
            alone.close()
        for i, (g, w) in enumerate(zip(got[c], want)):
            assert same(g, w), f"call {c} plane {i} differs from the call alone"
        assert any(w.any() for w in want) and not all((w == 255).all() for w in want)  # (a mask with both values)
