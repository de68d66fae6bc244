"""The numpy spec of ImageUnpack (tests/image_unpack_ref.py) against the known answers of the reference's own ImageRead tests
(tests/golden/image_unpack_goldens.json) and, where PIL is installed, against a decoder's own channel split of images written to disk."""
import numpy as np
import pytest

import image_unpack_ref as iu


@pytest.mark.parametrize("name", iu.golden_names())
def test_the_spec_reproduces_the_golden(name):
    packed, layout, bits, pal, want = iu.golden_case(name)
    p, a = iu.unpack(packed, layout, bits, pal)
    got = {f"p{k}": v for k, v in enumerate(p)}
    if a is not None:
        got["a"] = a
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


def test_the_goldens_cover_what_the_reference_tests():
    assert set(iu.golden_names()) == {"gray8", "gray16", "rgb24", "rgb48", "palette", "palette_indexed1", "palette_indexed2", "palette_indexed4", "rgba32", "gray8_alpha",
                                      "gray16_alpha", "rgba64", "gray1", "gray2", "gray4", "bmp_bgr24"}


def test_every_required_combination_has_content_and_a_spec():
    for combo in iu.COMBOS:
        layout, dt, bits = combo
        a = iu.content(3, 5, 70, combo)
        assert a.shape == (5, 70, iu.CHANNELS[layout]) and a.dtype == np.dtype(dt)
        p, al = iu.unpack(a, layout, bits, iu.palette() if layout == iu.INDEXED else None)
        assert len(p) == (1 if layout in (iu.GRAY, iu.GRAY_ALPHA) else 3) and (al is not None) == iu.HAS_ALPHA[layout]
        assert all(q.shape == (5, 70) and q.dtype == np.dtype(dt) for q in p + ([al] if al is not None else []))
        if layout == iu.INDEXED:
            assert len(np.unique(a)) == 256
        if np.dtype(dt) == np.float32:
            b = iu.bits_of(a)
            assert (b == 0x7FC00001).any() and (b == 0xFF800000).any() and (b >> 31).any()
            assert np.array_equal(iu.bits_of(p[1]), b[:, :, 1])  # as bits: the NaN payloads are kept
        elif bits >= 8:
            assert a.min() == 0 and a.max() == np.iinfo(dt).max


MODES = [("L", np.uint8, iu.GRAY), ("LA", np.uint8, iu.GRAY_ALPHA), ("RGB", np.uint8, iu.RGB), ("RGBA", np.uint8, iu.RGBA), ("P", np.uint8, iu.INDEXED), ("I;16", np.uint16, iu.GRAY)]


@pytest.mark.parametrize("mode,dt,layout", MODES, ids=[m[0] for m in MODES])
def test_a_decoded_image_unpacks_to_the_decoders_own_channel_split(tmp_path, mode, dt, layout):
    Image = pytest.importorskip("PIL.Image")
    h, w = 7, 13
    combo = (layout, dt, np.dtype(dt).itemsize * 8)
    src = iu.content(11, h, w, combo)
    pal = None
    if mode == "P":
        src = (np.arange(h * w, dtype=np.uint32).reshape(h, w, 1) * 37 % 256).astype(np.uint8)
        pal = iu.palette(2)
        pal[:, 3] = 255
        im = Image.frombytes("P", (w, h), src.tobytes())
        im.putpalette(pal[:, :3].tobytes())
    else:
        im = Image.fromarray(src[:, :, 0] if src.shape[2] == 1 else src)  # the mode follows from shape and type
        assert im.mode == mode
    path = tmp_path / f"{mode.replace(';', '')}.png"
    im.save(path)
    dec = Image.open(path)
    dec.load()
    assert dec.mode in (mode, "I;16", "I;16B"), dec.mode
    if mode == "P":
        packed = np.asarray(dec).astype(np.uint8)[:, :, None]
        table = np.frombuffer(bytes(dec.getpalette()), np.uint8).reshape(-1, 3)
        dpal = np.zeros((256, 4), np.uint8)
        dpal[:len(table), :3], dpal[:, 3] = table, 255
        want = [np.asarray(c) for c in dec.convert("RGB").split()]
        p, a = iu.unpack(packed, layout, 8, dpal)
        assert (a == 255).all()
    else:
        packed = np.asarray(dec).astype(dt)
        packed = packed[:, :, None] if packed.ndim == 2 else packed
        assert np.array_equal(packed, src)  # the file round trip is lossless
        want = [np.asarray(c).astype(dt) for c in dec.split()]
        p, a = iu.unpack(np.ascontiguousarray(packed), layout)
        if a is not None:
            p = p + [a]
    assert len(p) == len(want)
    for k, (x, y) in enumerate(zip(p, want)):
        assert x.shape == y.shape and np.array_equal(x, y), (mode, k)
