"""CPU: the Checkmate parity spec (tests/checkmate_ref.py) reproduces every key of the reference's
tests/goldens/checkmate.json (tests/golden/checkmate_goldens.json) and the numbers hard-coded in the reference's
tests/test_checkmate.py from tests/fixtures.py's inputs; its inputs reach the branches the natural fixture never does;
and libvszip_hip.so exports the entry point."""
import ctypes

import numpy as np
import pytest

import checkmate_ref as ck
import fixtures as fx

KEYS = sorted(ck.goldens())


def _avg(a):
    return fx.plane_stats(a)["avg"]


def binary_noise(seed, shape):
    """independent 0 / 255 samples"""
    return np.where(fx.splitmix64_plane(seed, shape, np.uint8) & 1, 255, 0).astype(np.uint8)


def correlated_clip(seed, shape, nframes):
    """frames that differ from a full-range base by -6 .. 6 per sample: the temporal tests pass or fail sample by sample"""
    base = fx.splitmix64_plane(seed, shape, np.uint8).astype(np.int32)
    return [np.clip(base + fx.splitmix64_plane(seed + 100 + k, shape, np.uint8).astype(np.int32) % 13 - 6, 0, 255).astype(np.uint8) for k in range(nframes)]


def test_all_25_keys_are_committed():
    assert len(KEYS) == 25
    assert sum(len(v) for v in ck.goldens().values()) == 39
    assert {ck.parse_key(k)[0] for k in KEYS} == {"GRAY8", "RGB24", "YUV420P8", "YUV422P8", "YUV444P8"}
    assert {ck.parse_key(k)[2]["tthr2"] > 0 for k in KEYS} == {True, False}  # both getFrame forms


@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_golden(key):
    want = ck.goldens()[key]
    outs = ck.run_key(key)
    assert len(outs) == len(want)
    for i, o in enumerate(outs):
        st, g = fx.plane_stats(o), want[f"p{i}"]
        assert st["min"] == g["min"] and st["max"] == g["max"], (key, i, st, g)
        assert st["avg"] == pytest.approx(g["avg"], rel=1e-9, abs=0), (key, i)


# reference tests/test_checkmate.py: frame-1 averages of the GRAY8 temporal clip
@pytest.mark.parametrize("args,expected", [
    (dict(thr=12, tmax=12, tthr2=0), 0.4871367378982843),
    (dict(thr=14, tmax=11, tthr2=4), 0.48752056525735293),
])
def test_reference_frame1_averages(args, expected):
    clip = [p[0] for p in ck.golden_inputs("GRAY8", "full")]
    assert _avg(ck.checkmate_clip(clip, **args)[1]) == pytest.approx(expected, rel=1e-6, abs=0)


def test_natural_fixture_reaches_neither_a_negative_curr_nor_saturation():
    f0, f1, f2 = (p[0] for p in ck.golden_inputs("GRAY8", "full"))
    for thr, tmax in ((12, 12), (255, 255), (0, 1)):
        m = ck.intermediates(f0, f1, f2, thr, tmax)
        assert m["curr"].min() >= 0 and m["out"].min() >= 0 and m["out"].max() <= 255


def test_binary_noise_reaches_every_extreme():
    """a condition on the input the GPU suites reuse: the most negative curr, an output below 0 and one above 255 before saturation"""
    p, c, n = (binary_noise(s, (64, 64)) for s in (11, 12, 13))
    m = ck.intermediates(p, c, n, 255, 255)
    assert m["curr"].min() == -1020 and m["curr"].max() == 6120
    assert m["out"].min() < 0 and m["out"].max() > 255
    out = ck.checkmate(None, p, c, n, None, 255, 255, 0)
    assert out.min() == 0 and out.max() == 255
    assert m["cw"].min() >= 0 and m["nw"].max() == 8192 and m["pw"].max() == 8192


def test_truncating_division():
    """curr = -1004 gives -100 (floor would give -101)"""
    c = np.zeros((5, 5), np.uint8)
    c[0, [0, 4]] = 255
    c[4, [0, 4]] = 255  # x = 2: curr = -(255 * 4) = -1020
    far = np.full((5, 5), 255, np.uint8)  # neighbours far away: both weights 0
    far[:, 2] = np.where(np.arange(5) % 4 == 0, 0, 255)
    m = ck.intermediates(far, c, far, 0, 1)
    assert m["curr"][0, 2] == -1020 and m["nw"][0, 2] == 0 and m["pw"][0, 2] == 0
    assert m["out"][0, 2] == (16384 * -102) >> 15 == -51
    c[2, 2] = 1  # curr = -1020 + 2 * 2 + 12 = -1004 -> -100, not floor's -101
    m = ck.intermediates(far, c, far, 0, 1)
    assert m["curr"][0, 2] == -1004 and m["out"][0, 2] == (m["cw"][0, 2] * -100 + m["pw"][0, 2] * 256 + m["nw"][0, 2] * 256) >> 15


def test_branch_mix_with_tthr2():
    shape = (64, 96)
    f = correlated_clip(5, shape, 5)
    frac = lambda t: ck.blend_mask(f[0], f[1], f[2], f[3], f[4], t).mean()
    assert 0.10 <= frac(8) <= 0.90
    assert frac(1) < 0.01
    assert frac(13) == 1.0 and frac(256) == 1.0
    blended = ck.checkmate(f[0], f[1], f[2], f[3], f[4], 12, 12, 13)
    a, c, b = (f[k][2:-2].astype(np.int32) for k in (1, 2, 3))
    assert np.array_equal(blended[2:-2], ((a + 2 * c + b) >> 2).astype(np.uint8))
    spatial = ck.checkmate(None, f[1], f[2], f[3], None, 12, 12, 0)
    mixed = ck.checkmate(f[0], f[1], f[2], f[3], f[4], 12, 12, 8)
    mask = np.zeros(shape, bool)
    mask[2:-2] = ck.blend_mask(f[0], f[1], f[2], f[3], f[4], 8)
    assert np.array_equal(mixed[mask], blended[mask]) and np.array_equal(mixed[~mask], spatial[~mask])


@pytest.mark.parametrize("nframes", [1, 2, 3, 6])
@pytest.mark.parametrize("tthr2", [0, 8])
def test_clip_end_clamping(nframes, tthr2):
    f = correlated_clip(9, (12, 21), nframes)
    hand = {1: [(0, 0, 0, 0)], 2: [(0, 0, 1, 1), (0, 0, 1, 1)], 3: [(0, 0, 1, 2), (0, 0, 2, 2), (0, 1, 2, 2)],
            6: [(0, 0, 1, 2), (0, 0, 2, 3), (0, 1, 3, 4), (1, 2, 4, 5), (2, 3, 5, 5), (3, 4, 5, 5)]}[nframes]
    got = ck.checkmate_clip(f, 12, 12, tthr2)
    assert len(got) == nframes
    for n, (a2, a1, b1, b2) in enumerate(hand):
        assert np.array_equal(got[n], ck.checkmate(f[a2], f[a1], f[n], f[b1], f[b2], 12, 12, tthr2)), n
    lists = ck.checkmate_clip([[p, p[:6, :5].copy()] for p in f], 12, 12, tthr2)  # frames as lists of planes
    assert all(np.array_equal(l[0], g) for l, g in zip(lists, got))


@pytest.mark.parametrize("kw,shape,msg", [
    (dict(tmax=0), (8, 8), r"Checkmate: tmax value should be in range \[1;255\]\."),
    (dict(tmax=256), (8, 8), r"Checkmate: tmax value should be in range \[1;255\]\."),
    (dict(tthr2=-1), (8, 8), r"Checkmate: tthr2 should be non-negative\."),
    (dict(thr=-1), (8, 8), r"Checkmate: thr value should be in range \[0;255\]\."),
    (dict(thr=256), (8, 8), r"Checkmate: thr value should be in range \[0;255\]\."),
    (dict(), (4, 8), r"Checkmate: clip too small; every plane must be at least 3 wide and 5 tall\."),
    (dict(), (8, 2), r"Checkmate: clip too small; every plane must be at least 3 wide and 5 tall\."),
    # the order of the checks: tmax, tthr2, thr, size
    (dict(tmax=0, tthr2=-1, thr=-1), (4, 2), "tmax value"),
    (dict(tthr2=-1, thr=-1), (4, 2), "tthr2 should"),
    (dict(thr=300), (4, 2), "thr value"),
])
def test_argument_errors(kw, shape, msg):
    a = np.zeros(shape, np.uint8)
    with pytest.raises(ValueError, match=msg):
        ck.checkmate(a, a, a, a, a, **kw)
    with pytest.raises(ValueError, match=msg):
        ck.check_checkmate_args([(16, 16), shape], kw.get("thr", 12), kw.get("tmax", 12), kw.get("tthr2", 0))


def test_smallest_plane_is_accepted():
    a = fx.splitmix64_plane(3, (5, 3), np.uint8)
    out = ck.checkmate(a, a, a, a, a, 12, 12, 4)
    assert out.shape == (5, 3) and np.array_equal(out[[0, 1, 3, 4]], a[[0, 1, 3, 4]])


@pytest.mark.parametrize("shape", [(5, 3), (6, 17), (9, 33), (40, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("tthr2", [0, 300])
def test_edge_rows_equal_the_source(shape, tthr2):
    f = [fx.splitmix64_plane(20 + k, shape, np.uint8) for k in range(5)]
    out = ck.checkmate(f[0], f[1], f[2], f[3], f[4], 12, 12, tthr2)
    rows = [0, 1, shape[0] - 2, shape[0] - 1]
    assert np.array_equal(out[rows], f[2][rows])
    if shape[0] > 5:
        assert not np.array_equal(out[2:-2], f[2][2:-2])


def test_library_exports_the_entry_point():
    from vszip_amd import capi

    lib = ctypes.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "vszip_checkmate")
    assert "vszip_checkmate" in capi.SYMBOLS and len(capi.SYMBOLS["vszip_checkmate"][1]) == 7
    assert capi.load().vszip_abi_version() == 4
    assert all(hasattr(capi.Device, n) for n in ("checkmate", "prepared_checkmate", "checkmate_clip"))
    assert ctypes.sizeof(capi.TemporalNbrs) == 8 * ctypes.sizeof(ctypes.c_void_p)
