"""vszip_color_map_lut (device-free, csrc/host_params.cpp) against the numpy spec (tests/color_map_ref.py), bit for bit: the four analytic
palettes, the reference's end points, every table length the reference has plus the edges, random palettes; palettes on which a fused
interpolation would give another byte; the argument errors; and the five reference goldens through spec and library table."""
import numpy as np
import pytest

import color_map_ref as cm
import fixtures as fx
from vszip_amd import capi
from vszip_amd.capi import VszipError


def lib_lut(r, g, b):
    t = capi.color_map_lut(r, g, b)
    assert t.dtype == np.uint8 and t.shape == (3, 256)
    return t


@pytest.mark.parametrize("name", sorted(cm.ANALYTIC))
def test_analytic_palettes(name):
    pal = cm.analytic_palette(name)
    assert all(len(c) == cm.ANALYTIC[name][1] and c.dtype == np.float32 for c in pal)
    assert np.array_equal(lib_lut(*pal), cm.lut(*pal))


def test_autumn_end_points():
    t = lib_lut(*cm.analytic_palette("autumn"))
    assert tuple(int(v) for v in t[:, 0]) == (255, 0, 0) and tuple(int(v) for v in t[:, 255]) == (255, 255, 0)


@pytest.mark.parametrize("n", cm.LENGTHS)
def test_random_palettes_of_every_length(n):
    rng = np.random.default_rng(1000 + n)
    for k in range(200):
        pal = rng.random((3, n), dtype=np.float32)
        if k % 4 == 0:  # the ends of the range, too
            pal[rng.integers(3), rng.integers(n)] = np.float32(k % 8 == 0)
        assert np.array_equal(lib_lut(*pal), cm.lut(*pal)), (n, k)


@pytest.mark.parametrize("n", cm.LENGTHS)
def test_ramps_of_every_length(n):
    t = (np.arange(n, dtype=np.float64) / max(n - 1, 1)).astype(np.float32)
    pal = (t, (np.float32(1) - t).astype(np.float32), (t * t).astype(np.float32))
    got = lib_lut(*pal)
    assert np.array_equal(got, cm.lut(*pal))
    if n >= 2:
        assert got[0, 0] == 0 and got[0, 255] == 255 and got[1, 0] == 255 and got[1, 255] == 0


def test_the_interpolation_is_not_contracted():
    """two-point palettes on which fma(d, frac, lo) and the reference's separately rounded multiply and add give different bytes"""
    pairs = np.random.default_rng(0).random((20000, 2), dtype=np.float32)
    found = []
    for a, b in pairs:
        pal = np.array([a, b], np.float32)
        plain, fused = cm.lut(pal, pal, pal), cm.lut(pal, pal, pal, contracted=True)
        if not np.array_equal(plain, fused):
            found.append((pal, plain))
    assert len(found) >= 1
    for pal, plain in found:
        assert np.array_equal(lib_lut(pal, pal, pal), plain), pal.tolist()
    pal = np.array([0.20607343316078186, 0.6694883108139038], np.float32)
    plain = cm.lut(pal, pal, pal)
    assert not np.array_equal(plain, cm.lut(pal, pal, pal, contracted=True))
    assert np.array_equal(lib_lut(pal, pal, pal), plain)


def test_argument_errors():
    e = np.zeros(0, np.float32)
    with pytest.raises(VszipError, match=r"ColorMap: len = 0") as ei:
        capi.color_map_lut(e, e, e)
    assert ei.value.code == capi.ERR_ARG
    ok = np.linspace(0, 1, 11, dtype=np.float32)
    for ch, name in enumerate("rgb"):
        for bad, where in ((np.float32("nan"), 4), (np.float32(1.01), 10), (np.float32(-0.01), 0), (np.float32("inf"), 7)):
            pal = [ok.copy() for _ in range(3)]
            pal[ch][where] = bad
            with pytest.raises(VszipError, match=rf"ColorMap: {name}: table entry (\d+) \(palette points (\d+) and (\d+)\)") as ei:
                capi.color_map_lut(*pal)
            assert ei.value.code == capi.ERR_ARG
            with pytest.raises(ValueError, match=rf"{name}: table entry (\d+)") as si:
                cm.lut(*pal)
            assert str(si.value).split("entry ")[1] in str(ei.value).split("(")[0], (str(si.value), str(ei.value))  # the same entry as the spec's
            lo, hi = (int(v) for v in __import__("re").search(r"points (\d+) and (\d+)", str(ei.value)).groups())
            assert where in (lo, hi), (where, str(ei.value))
    assert np.array_equal(lib_lut(ok, ok, ok), cm.lut(ok, ok, ok))  # and a valid call afterwards goes through
    # values a little outside 0..1 that still land on 0..255 are served, as in the reference
    edge = np.array([-0.0015, 1.0015], np.float32)
    assert np.array_equal(lib_lut(edge, edge, edge), cm.lut(edge, edge, edge))


@pytest.mark.parametrize("key", sorted(cm.goldens()))
def test_goldens_through_spec_and_library_table(key):
    assert len(cm.goldens()) == 5
    y, color = cm.golden_input(key)
    pal = cm.palette_of_color(color)
    table = lib_lut(*pal)
    assert np.array_equal(table, cm.lut(*pal))
    for i, o in enumerate(cm.apply(y, table)):
        st, g = fx.plane_stats(o), cm.goldens()[key][f"p{i}"]
        assert st["min"] == g["min"] and st["max"] == g["max"] and st["avg"] == pytest.approx(g["avg"], rel=1e-12, abs=0), (key, i, st, g)
