"""vszip_chain_ops: chains over every frame-in / frame-out filter on resident planes in one call, bit-identical to the same entry points called one
after another with explicit intermediate planes (include/vszip_hip.h, "vszip_chain_ops"). Planes are 120 x 208 luma + 60 x 104
chroma. The twins are the library's own entry points, so that equality alone could hide two equally wrong answers: the CLAHE -> Limiter chain is
anchored, intermediate and result, against tests/clahe_ref.py and the CPU oracle."""
import numpy as np
import pytest

import fixtures as fx

pytestmark = pytest.mark.gpu

SHAPES = [(120, 208), (60, 104), (60, 104)]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def same(got, want) -> bool:
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def clip(dtype, frames, shapes=SHAPES, seed=0):
    """frames x planes of natural content, each frame shifted a little against the one before (neighbouring frames are alike, not equal)"""
    out = []
    for f in range(frames):
        planes = []
        for p, s in enumerate(shapes):
            a = np.roll(fx.tiled_natural(s, dtype, p), (f + seed, 2 * f + seed), axis=(0, 1))
            n = fx.splitmix64_plane(100 * seed + 10 * f + p, s, dtype)
            a = a // 8 * 7 + n // 16 if np.dtype(dtype).kind == "u" else a * np.float32(0.9) + n * np.float32(0.05)
            planes.append(np.ascontiguousarray(a.astype(dtype)))
        out.append(planes)
    return out


def resident(dev, frames):
    """-> flat (host planes, device planes, empty destinations, slots, frame numbers), frame-major"""
    host = [p for fr in frames for p in fr]
    slots = [k for fr in frames for k in range(len(fr))]
    nums = [f for f, fr in enumerate(frames) for _ in fr]
    return host, [dev.upload(p) for p in host], [dev.empty(p.shape[0], p.shape[1], p.dtype) for p in host], slots, nums


def fresh(dev, like, which=None):
    """new planes for the entries in `which` (all by default); the others keep the plane they have (a stage that passes them through)"""
    return [dev.empty(p.h, p.w, p.dtype) if which is None or i in which else p for i, p in enumerate(like)]


def by_frame(flat, per=3):
    return [flat[i:i + per] for i in range(0, len(flat), per)]


def test_u8_temporal_chain_equals_sequential_calls(dev):
    """Checkmate(tthr2 = 8) -> Compress(chroma on) -> MosquitoNR(luma only) -> CombMask(mthresh = 9) over four frames: n +- 2 clamps at both ends, and
    frame 1 / 2 have neighbours that are all different planes but one"""
    from vszip_amd import capi

    host, ds, dd, slots, nums = resident(dev, clip(np.uint8, 4))
    tb = capi.compress_tables(codec=1, quality=35)
    chroma = [int(s > 0) for s in slots]
    ops = [{"checkmate": dict(tthr2=8)}, {"compress": tb, "chroma": chroma}, {"mosquito_nr": dict(strength=20), "planes": (True, False, False)}, {"comb_mask": dict(mthresh=9)}]
    dev.chain_ops(ops, ds, dd, slots, frames=nums)
    got = [dev.download(d) for d in dd]
    # the twin: every intermediate a plane of its own
    a = fresh(dev, ds)
    dev.checkmate_clip(by_frame(ds), by_frame(a), tthr2=8)
    b = fresh(dev, a)
    dev.compress(a, b, tb, chroma)
    luma = [i for i, s in enumerate(slots) if s == 0]
    c = fresh(dev, b, luma)
    dev.mosquito_nr([b[i] for i in luma], [c[i] for i in luma], strength=20)
    e = fresh(dev, c)
    dev.comb_mask(c, e, [c[max(i - 3, i % 3)] for i in range(len(c))], mthresh=9)
    want = [dev.download(p) for p in e]
    for i in range(len(host)):
        assert same(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    assert not want[0].any() and any(w.any() for w in want[3:])  # frame 0 is its own previous frame: no motion; later frames have some
    stages = [[dev.download(p) for p in st] for st in (a, b, c)]
    assert not same(stages[0][0], host[0]) and not same(stages[1][4], stages[0][4]) and not same(stages[2][3], stages[1][3])  # every stage did something


def test_u16_chain_with_per_frame_grain_equals_sequential_calls(dev):
    """BoxBlur(luma) -> MosquitoNR(bits 16) -> Deband(sample mode 2, dynamic grain: the two frames read the grain buffers at different offsets) ->
    Limiter(chroma) over two frames"""
    from vszip_amd import capi

    host, ds, dd, slots, nums = resident(dev, clip(np.uint16, 2))
    tab = capi.deband_tables(208, 120, ssw=1, ssh=1, num_frames=2, range=15, sample_mode=2, seed=5, grain=(4112, 2056), dynamic_grain=True)
    assert int(tab["grain_offsets"][0]) != int(tab["grain_offsets"][1])
    rt = dev.upload_deband_tables(tab)
    entries = []
    for s, f in zip(slots, nums):
        y = s == 0
        entries.append(dev.deband_entry(rt["luma" if y else "chroma"], 0 if y else 1, 0 if y else 1, rt["grain_y" if y else "grain_c"], int(tab["grain_offsets"][f]),
                                        208 if y else 112, 48 * 257, 80 * 257, 20 * 257, 4096, 60160))
    lo, hi = [0.0, 20000.0, 20000.0], [65535.0, 45000.0, 45000.0]
    ops = [{"boxblur": (2, 1, 2, 1), "planes": (True, False, False)}, {"mosquito_nr": dict(strength=24, restore=100)},
           {"deband": entries, "sample_mode": 2, "max_offset": tab["max_offset"]}, {"limiter": (lo, hi), "planes": (False, True, True)}]
    dev.chain_ops(ops, ds, dd, slots, bits=16)
    got = [dev.download(d) for d in dd]
    luma = [i for i, s in enumerate(slots) if s == 0]
    chroma = [i for i, s in enumerate(slots) if s != 0]
    a = fresh(dev, ds, luma)
    dev.boxblur([ds[i] for i in luma], [a[i] for i in luma], 2, 1, 2, 1)
    b = fresh(dev, a)
    dev.mosquito_nr(a, b, strength=24, restore=100, bits=16)
    c = fresh(dev, b)
    dev.deband(b, c, entries, 2, True, 1.5, 0.15, tab["max_offset"])
    e = fresh(dev, c, chroma)
    dev.limiter([c[i] for i in chroma], [e[i] for i in chroma], [lo[slots[i]] for i in chroma], [hi[slots[i]] for i in chroma])
    want = [dev.download(p) for p in e]
    for i in range(len(host)):
        assert same(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    # the grain offset is the frame's: with frame 1's entries on frame 0's planes the luma differs
    swapped = fresh(dev, b[:3])
    dev.deband(b[:3], swapped, entries[3:], 2, True, 1.5, 0.15, tab["max_offset"])
    assert not same(dev.download(swapped[0]), dev.download(c[0]))
    assert not same(dev.download(b[1]), dev.download(c[1])) and not same(dev.download(c[1]), want[1])


def test_f32_chain_equals_sequential_calls(dev):
    """BilateralDither(default radius 16, sub-sampled) -> Deband(sample mode 7: the angle planes go through the scratch) -> BoxBlur, one frame"""
    from vszip_amd import capi

    host, ds, dd, slots, _ = resident(dev, clip(np.float32, 1))
    prm = capi.bilateral_dither_params(True, 32, radius=16, subspl=0.0)
    assert prm["subsampled"] and prm["K"] > 0
    pts = dev.upload_bilateral_dither_points(capi.bilateral_dither_points(16, 0.0))
    bd = [dev.bilateral_dither_entry(16, prm["m"], prm["wmax"], prm["sum_w_min"], pts, prm["K"]) for _ in slots]
    tab = capi.deband_tables(208, 120, ssw=1, ssh=1, num_frames=1, range=15, sample_mode=7, seed=3, is_float=True)
    rt = dev.upload_deband_tables(tab)
    de = [dev.deband_entry(rt["luma" if s == 0 else "chroma"], int(s > 0), int(s > 0), None, 0, 0, 48 / 255, 80 / 255, 20 / 255, 0.0, 1.0) for s in slots]
    ops = [{"bilateral_dither": bd}, {"deband": de, "sample_mode": 7, "max_offset": tab["max_offset"]}, {"boxblur": (3, 1, 3, 1)}]
    dev.chain_ops(ops, ds, dd, slots)
    got = [dev.download(d) for d in dd]
    a = fresh(dev, ds)
    dev.bilateral_dither(ds, a, bd)
    b = fresh(dev, a)
    dev.deband(a, b, de, 7, True, 1.5, 0.15, tab["max_offset"])
    c = fresh(dev, b)
    dev.boxblur(b, c, 3, 1, 3, 1)
    want = [dev.download(p) for p in c]
    for i in range(len(host)):
        assert same(got[i], want[i]), i
    assert not same(dev.download(a[0]), host[0]) and not same(dev.download(b[0]), dev.download(a[0]))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_clahe_limiter_chain_equals_sequential_calls_and_the_specification(dev, oracle, dtype):
    """CLAHE(tiles 3 x 2) -> Limiter: against the twin, and both stages against tests/clahe_ref.py and the oracle's Limiter"""
    import clahe_ref as cr

    host, ds, dd, slots, _ = resident(dev, clip(dtype, 1))
    peak = float(np.iinfo(dtype).max)
    lo, hi = [float(int(peak * 0.1))] * 3, [float(int(peak * 0.8)), float(int(peak * 0.6)), float(int(peak * 0.6))]
    dev.chain_ops([{"clahe": (7, [3, 2])}, {"limiter": (lo, hi)}], ds, dd, slots)
    got = [dev.download(d) for d in dd]
    a = fresh(dev, ds)
    dev.clahe(ds, a, 7, [3, 2])
    b = fresh(dev, a)
    dev.limiter(a, b, [lo[s] for s in slots], [hi[s] for s in slots])
    for i, p in enumerate(host):
        mid = cr.clahe(p, 7, (3, 2))
        assert same(dev.download(a[i]), mid), i
        want = oracle.limiter(mid, lo[slots[i]], hi[slots[i]])
        assert same(dev.download(b[i]), want) and same(got[i], want), i
        assert not same(mid, p) and not same(want, mid)


def test_temporal_neighbours_are_what_the_previous_stage_left(dev):
    """BoxBlur -> Checkmate over four frames is Checkmate on the blurred clip - and not Checkmate on the blurred frame between the caller's unblurred
    neighbours, which the inputs can tell apart"""
    host, ds, dd, slots, nums = resident(dev, clip(np.uint8, 4, seed=2))
    order = [5, 0, 9, 2, 7, 4, 11, 6, 1, 8, 3, 10]  # the table is a clip in any order: neighbours are found by (slot, frame)
    pick = lambda l: [l[i] for i in order]
    dev.chain_ops([{"boxblur": (1, 1, 1, 1)}, {"checkmate": dict(thr=12, tmax=12, tthr2=6)}], pick(ds), pick(dd), pick(slots), frames=[n + 40 for n in pick(nums)])
    got = [dev.download(d) for d in dd]
    blurred = fresh(dev, ds)
    dev.boxblur(ds, blurred, 1, 1, 1, 1)
    out = fresh(dev, ds)
    dev.checkmate_clip(by_frame(blurred), by_frame(out), tthr2=6)
    want = [dev.download(p) for p in out]
    for i in range(len(host)):
        assert same(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    # the wrong reading: neighbours from the caller's planes
    _, p1, n1, p2, n2 = dev.clip_neighbours(by_frame(ds))
    wrong = fresh(dev, ds)
    dev.checkmate(blurred, wrong, p1, n1, p2, n2, tthr2=6)
    differ = [not same(dev.download(w), want[i]) for i, w in enumerate(wrong)]
    assert all(differ[0::3]), differ  # every luma plane tells the two apart


def test_per_entry_arrays_follow_their_entries(dev):
    """slots [0, 1, 2, 0, 1, 2], MosquitoNR on slot 0 only: entry 0 gets strength[0], entry 3 strength[3]; the entries of the skipped slots hold values
    the entry point would refuse, so they are not read"""
    host, ds, dd, slots, _ = resident(dev, clip(np.uint8, 2, seed=1))
    assert slots == [0, 1, 2, 0, 1, 2]
    strength, restore, radius = [6, 99, 99, 30, 99, 99], [128, -5, -5, 64, -5, -5], [2, 7, 7, 1, 7, 7]
    dev.chain_ops([{"mosquito_nr": dict(strength=strength, restore=restore, radius=radius, chroma=[0, 1, 1, 0, 1, 1]), "planes": (True, False, False)}], ds, dd, slots)
    got = [dev.download(d) for d in dd]
    for i in (0, 3):
        alone = fresh(dev, [ds[i]])
        dev.mosquito_nr([ds[i]], alone, strength=strength[i], restore=restore[i], radius=radius[i])
        assert same(got[i], dev.download(alone[0])), i
        other = fresh(dev, [ds[i]])
        dev.mosquito_nr([ds[i]], other, strength=strength[3 - i], restore=restore[3 - i], radius=radius[3 - i])
        assert not same(got[i], dev.download(other[0])), i  # (the other frame's parameters give another result)
    for i in (1, 2, 4, 5):
        assert same(got[i], host[i])  # passed through


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.float32], ids=["u16", "u8", "f32"])
def test_chain_run_and_chain_ops_agree(dev, dtype):
    """the stage list of tests/test_gpu_chain.py::test_chain_equals_sequential_calls through both entry points: identical bytes"""
    frames = 2
    src = [fx.tiled_natural(s, dtype, p) for _ in range(frames) for p, s in enumerate(SHAPES)]
    src = [np.ascontiguousarray(np.roll(a, 3 * i, axis=1)) for i, a in enumerate(src)]
    slots = [0, 1, 2] * frames
    is_f = np.dtype(dtype).kind == "f"
    hist = 65536 if is_f else 1 << (8 * np.dtype(dtype).itemsize)
    peak = float(hist - 1)
    cfg = dev.bilateral_cfg([2], [0.05], yuv=True, ssw=1, ssh=1, hist_len=hist)
    lo = [0.1, 0.2, 0.2] if is_f else [peak * 0.1, peak * 0.3, peak * 0.3]
    hi = [0.9, 0.6, 0.6] if is_f else [peak * 0.9, peak * 0.6, peak * 0.6]
    lo, hi = [float(int(v)) if not is_f else v for v in lo], [float(int(v)) if not is_f else v for v in hi]
    stages = [{"bilateral": cfg, "peak": peak}, {"boxblur": (3, 1, 3, 1), "planes": (True, False, False)}, {"limiter": (lo, hi), "planes": (False, True, True)},
              {"boxblur": (1, 2, 1, 1)}]
    ds = [dev.upload(a) for a in src]
    d1, d2 = fresh(dev, ds), fresh(dev, ds)
    dev.chain_run(stages, ds, d1, slots)
    dev.chain_ops(stages, ds, d2, slots)
    for i in range(len(src)):
        g1, g2 = dev.download(d1[i]), dev.download(d2[i])
        assert same(g1, g2) and not same(g1, src[i]), i
    dev.bilateral_free(cfg)
