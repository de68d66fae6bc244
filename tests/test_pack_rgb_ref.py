"""The numpy spec of vszip.PackRGB (tests/pack_rgb_ref.py) against the reference's recorded results: its six goldens, reproduced from the
committed crop, and the known answers of its 16 x 4 gradient in both formulas; and the wrap of an out-of-range 10-bit sample."""
import numpy as np
import pytest

import pack_rgb_ref as pr


@pytest.mark.parametrize("key", sorted(pr.goldens()))
def test_the_spec_gives_the_golden_statistics(key):
    assert len(pr.goldens()) == 6
    fmt, geom, _ = key.split("|")
    r, g, b, bits = pr.golden_inputs(fmt, geom)
    assert r.shape == {"full": (320, 640), "odd": (319, 639), "tiny": (7, 13)}[geom]
    packed = pr.pack(r, g, b, bits)
    assert packed.dtype == np.uint32 and packed.shape == r.shape
    st, want = pr.stats(packed), pr.goldens()[key]["p0"]
    assert st["min"] == want["min"] and st["max"] == want["max"] and st["avg"] == pytest.approx(want["avg"], rel=1e-12, abs=0), (key, st, want)


def _gradient():
    """the reference's 16 x 4 picture of known values (its tests/test_packrgb.py)"""
    rows = [[((x * 16 + y * 3) % 256, (255 - x * 9) % 256, (x * x + y) % 256) for x in range(16)] for y in range(4)]
    a = np.array(rows, np.uint8)  # (4, 16, 3)
    return np.ascontiguousarray(a[..., 0]), np.ascontiguousarray(a[..., 1]), np.ascontiguousarray(a[..., 2])


def test_rgb24_known_answers():
    r, g, b = _gradient()
    out = pr.pack(r, g, b, 8)
    for y in range(4):
        for x in range(16):
            assert int(out[y, x]) == int(b[y, x]) | (int(g[y, x]) << 8) | (int(r[y, x]) << 16) | (255 << 24)
    assert out.view(np.uint8).reshape(4, 16, 4)[2, 5].tolist() == [int(b[2, 5]), int(g[2, 5]), int(r[2, 5]), 255]  # in memory: B, G, R, 0xFF


def test_rgb30_known_answers():
    r, g, b = (p.astype(np.uint16) << 2 for p in _gradient())  # resize.Point to 10 bits: the value shifted
    out = pr.pack(r, g, b, 10)
    for y in range(4):
        for x in range(16):
            assert int(out[y, x]) == int(b[y, x]) | (int(g[y, x]) << 10) | (int(r[y, x]) << 20) | (0b11 << 30)


def test_a_16_bit_sample_wraps_as_the_uint32_expression_does():
    full, zero = np.full((1, 1), 65535, np.uint16), np.zeros((1, 1), np.uint16)
    assert int(pr.pack(full, zero, zero, 10)[0, 0]) == ((65535 << 20) | (3 << 30)) & 0xFFFFFFFF == 0xFFF00000
    assert int(pr.pack(zero, full, zero, 10)[0, 0]) == ((65535 << 10) | (3 << 30)) & 0xFFFFFFFF == 0xC3FFFC00
    assert int(pr.pack(zero, zero, full, 10)[0, 0]) == 65535 | (3 << 30)
    assert int(pr.pack(full, full, full, 10)[0, 0]) == 0xFFFFFFFF
    r, g, b = np.array([[1024]], np.uint16), np.array([[1]], np.uint16), np.array([[2047]], np.uint16)
    assert int(pr.pack(r, g, b, 10)[0, 0]) == (2047 | (1 << 10) | (1024 << 20) | (3 << 30)) & 0xFFFFFFFF  # b runs into g's field; r's bit 10 lands on bit 30


def test_the_rgb30_inputs_are_zimgs_full_range_conversion():
    a = pr.rgb30(np.arange(256, dtype=np.uint8).reshape(1, 16, 16))
    assert a.dtype == np.uint16 and int(a.min()) == 0 and int(a.max()) == 1023 and int(a[0, 8, 0]) == 514  # 128 -> 513.5 + 0.5
