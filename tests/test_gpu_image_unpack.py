"""GPU: vszip_image_unpack against the numpy spec (tests/image_unpack_ref.py), bit for bit, for every combination of layout, sample
type and source bits the reference's switch has: frames around every step of the kernel's mapping (a unit of 16 bytes a plane, a wave,
one sweep of the workgroup's 256 lanes) in one call, and more frames than one kernel-argument table holds; dense sources and rows with
a padded byte pitch; source bases 0 to 5 pixels into their allocation; output planes 16-byte aligned and deliberately misaligned; the
alpha channel dropped; INDEXED with 256 different palette entries; the reference's golden answers through the device; argument errors.

Every call works on two device allocations, one holding all sources and one all output planes, filled with 0xCD between the planes: after
the call the sources are unchanged and every byte of the output allocation outside `[0, w) x h` of the planes the call was given is
still 0xCD."""
import numpy as np
import pytest

import image_unpack_ref as iu
from vszip_amd.capi import VszipError

pytestmark = pytest.mark.gpu

# (3, 1031): longer than one sweep of the workgroup at four pixels a lane (1024); (2, 4117): at sixteen, too (4096)
SIZES = [(1, 1), (7, 13), (2, 16), (3, 64), (5, 17), (37, 83), (3, 1031), (2, 4117)]
FILL = 0xCD
ALPHA_COMBOS = [c for c in iu.COMBOS if iu.HAS_ALPHA[c[0]]]
ids = lambda combos: [iu.combo_id(c) for c in combos]


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def _up(n, a):
    return -(-n // a) * a


def run(dev, combo, packed, misaligned=False, pad=None, drop_alpha=False, pal=None):
    """one call on the frames `packed` (arrays of (h, w, channels)); -> per frame (colour planes, alpha or None) as downloaded, after the
    checks of the module's docstring. pad: source rows are padded to the next multiple of `pad` bytes, and by `pad` more"""
    layout, dt, bits = combo
    dt = np.dtype(dt)
    S, C = dt.itemsize, iu.CHANNELS[layout]
    pxb = S * C
    ncol, has_a = (1 if layout in (iu.GRAY, iu.GRAY_ALPHA) else 3), iu.HAS_ALPHA[layout]
    # sources: frame i starts i % 6 pixels into its own 64-byte aligned region
    src_at, pos = [], 0
    for i, p in enumerate(packed):
        h, w = p.shape[:2]
        pitch = w * pxb if pad is None else _up(w * pxb, pad) + pad
        start = _up(pos, 64) + (i % 6) * pxb
        src_at.append((start, pitch))
        pos = start + (h - 1) * pitch + w * pxb
    hsrc = np.full((1, _up(pos, 64)), 0x5A, np.uint8)
    for p, (start, pitch) in zip(packed, src_at):
        h, w = p.shape[:2]
        rows = iu.row_bytes(p)
        for y in range(h):
            hsrc[0, start + y * pitch:start + y * pitch + w * pxb] = rows[y]
    # outputs: aligned planes have 16-byte bases and pitches; misaligned ones start one sample off and have pitch w + 1
    out_at, pos = [], 0
    for p in packed:
        h, w = p.shape[:2]
        planes = []
        for _ in range(ncol + has_a):
            pitch = w + 1 if misaligned else _up(w * S, 16) // S
            start = _up(pos, 64) + (S if misaligned else 0)
            planes.append((start, pitch))
            pos = start + h * pitch * S
        out_at.append(planes)
    hout = np.full((1, _up(pos, 64)), FILL, np.uint8)
    dsrc, dout = dev.upload(hsrc), dev.upload(hout)
    view = lambda at, h, w: dev.wrap(dout.ptr + at[0], h, w, at[1], dt)
    srcs, planes, alphas = [], [], []
    for p, (start, pitch), at in zip(packed, src_at, out_at):
        h, w = p.shape[:2]
        srcs.append(dev.wrap(dsrc.ptr + start, h, w * pxb, pitch, np.uint8))
        planes.append([view(a, h, w) for a in at[:ncol]])
        alphas.append(view(at[ncol], h, w) if has_a and not drop_alpha else None)
    dev.image_unpack(srcs, planes, alphas, layout, bits, pal)
    got_src, got = dev.download(dsrc), dev.download(dout)
    assert np.array_equal(got_src, hsrc), "the sources were written"
    untouched = np.ones(got.shape[1], bool)
    res = []
    for i, (p, at) in enumerate(zip(packed, out_at)):
        h, w = p.shape[:2]
        one = []
        for k, (start, pitch) in enumerate(at):
            if k == ncol and drop_alpha:
                one.append(None)
                continue
            a = got[0, start:start + h * pitch * S].view(dt).reshape(h, pitch)[:, :w]
            untouched[start:start + h * pitch * S].reshape(h, pitch * S)[:, :w * S] = False
            one.append(a)
        res.append((one[:ncol], one[ncol] if has_a else None))
    bad = np.flatnonzero(untouched & (got[0] != FILL))
    assert bad.size == 0, f"{bad.size} bytes outside the planes were written, the first at {int(bad[0])}"
    dsrc.free()
    dout.free()
    return res


def check(dev, combo, sizes, seed=0, pal=None, **kw):
    layout, dt, bits = combo
    if layout == iu.INDEXED and pal is None:
        pal = iu.palette(seed)
    packed = [iu.content(seed + i, h, w, combo) for i, (h, w) in enumerate(sizes)]
    res = run(dev, combo, packed, pal=pal, **kw)
    for i, (p, (gp, ga)) in enumerate(zip(packed, res)):
        wp, wa = iu.unpack(p, layout, bits, pal, alpha=not kw.get("drop_alpha", False))
        assert len(gp) == len(wp) and (ga is None) == (wa is None)
        for k, (g, x) in enumerate(zip(gp + ([ga] if ga is not None else []), wp + ([wa] if wa is not None else []))):
            assert g.shape == x.shape and np.array_equal(iu.bits_of(g), iu.bits_of(x)), (iu.combo_id(combo), i, p.shape, k, int((iu.bits_of(g) != iu.bits_of(x)).sum()))
    return res


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned16", "misaligned"])
@pytest.mark.parametrize("combo", iu.COMBOS, ids=ids(iu.COMBOS))
def test_every_size_in_one_call(dev, combo, misaligned):
    check(dev, combo, SIZES, seed=1, misaligned=misaligned)


@pytest.mark.parametrize("combo", iu.COMBOS, ids=ids(iu.COMBOS))
def test_more_frames_than_one_table_holds(dev, combo):
    """200 frames: the batching loop of plane_table.hpp runs twice (a table holds 192)"""
    sizes = [(1 + i % 5, 1 + (i * 7) % 41) for i in range(200)]
    check(dev, combo, sizes, seed=2, misaligned=False)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned16", "misaligned"])
@pytest.mark.parametrize("pad", [4, 64])
@pytest.mark.parametrize("combo", [(iu.RGB, np.uint8, 8), (iu.RGB, np.uint16, 16)], ids=["rgb24", "rgb48"])
def test_padded_byte_pitch(dev, combo, pad, misaligned):
    """rows padded as a BMP's are (to 4 bytes, and 4 more), and to 64: the planes equal the spec, which never saw the padding"""
    check(dev, combo, SIZES, seed=3, misaligned=misaligned, pad=pad)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned16", "misaligned"])
@pytest.mark.parametrize("combo", ALPHA_COMBOS, ids=ids(ALPHA_COMBOS))
def test_without_an_alpha_plane_the_colour_planes_are_the_same_and_nothing_else_is_written(dev, combo, misaligned):
    full = check(dev, combo, SIZES, seed=4, misaligned=misaligned)
    dropped = check(dev, combo, SIZES, seed=4, misaligned=misaligned, drop_alpha=True)  # (run() sees the alpha planes' memory keep its fill)
    for (p0, a0), (p1, a1) in zip(full, dropped):
        assert a0 is not None and a1 is None
        for x, y in zip(p0, p1):
            assert np.array_equal(iu.bits_of(x), iu.bits_of(y))


def test_indexed_with_256_different_entries_on_an_image_that_uses_every_index(dev):
    combo = (iu.INDEXED, np.uint8, 8)
    pal = iu.palette(9)
    assert len(np.unique(iu.content(5, 5, 64, combo))) == 256
    check(dev, combo, [(5, 64), (16, 16), (1, 300)], seed=5, pal=pal)
    check(dev, combo, [(5, 64), (16, 16), (1, 300)], seed=5, pal=pal, misaligned=True)


@pytest.mark.parametrize("name", iu.golden_names())
def test_golden_pixels_through_the_device_give_the_golden_planes(dev, name):
    packed, layout, bits, pal, want = iu.golden_case(name)
    for misaligned in (False, True):
        (p, a), = run(dev, (layout, packed.dtype, bits), [packed], misaligned=misaligned, pal=pal)
        got = {f"p{k}": v for k, v in enumerate(p)}
        if a is not None:
            got["a"] = a
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


def test_argument_errors(dev):
    h, w = 6, 20
    mk = lambda dt: dev.upload(np.full((h, w), 7, dt))
    src = dev.upload(np.zeros((h, w * 16), np.uint8))
    p8, p16, p32 = [mk(np.uint8) for _ in range(4)], [mk(np.uint16) for _ in range(4)], [mk(np.float32) for _ in range(4)]
    pal = iu.palette(0)
    view = lambda pxb: dev.wrap(src.ptr, h, w * pxb, w * pxb, np.uint8)

    def refused(match, srcs, planes, alphas, layout, bits=None, palette=None):
        with pytest.raises(VszipError, match=match) as ei:
            dev.image_unpack(srcs, planes, alphas, layout, bits, palette)
        assert ei.value.code == -1

    # combinations that are not served
    refused("ImageUnpack: BGR with type 1 and 16 source bits is not served", [view(6)], [p16[:3]], [None], iu.BGR)
    refused("ImageUnpack: BGRA with type 1 and 16 source bits is not served", [view(8)], [p16[:3]], [p16[3]], iu.BGRA)
    refused("ImageUnpack: RGB with type 3 and 32 source bits is not served", [view(12)], [p32[:3]], [None], iu.RGB)
    refused("ImageUnpack: GRAY with type 3 and 32 source bits is not served", [view(4)], [p32[:1]], [None], iu.GRAY)
    refused("ImageUnpack: GRAY with type 0 and 3 source bits is not served", [view(1)], [p8[:1]], [None], iu.GRAY, 3)
    refused("ImageUnpack: GRAY with type 1 and 4 source bits is not served", [view(2)], [p16[:1]], [None], iu.GRAY, 4)
    refused("ImageUnpack: RGB with type 0 and 4 source bits is not served", [view(3)], [p8[:3]], [None], iu.RGB, 4)
    refused("ImageUnpack: RGBA with type 1 and 8 source bits is not served", [view(8)], [p16[:3]], [p16[3]], iu.RGBA, 8)
    refused("ImageUnpack: layout 7 is not one of", [view(3)], [p8[:3]], [None], 7)
    refused("ImageUnpack: layout -1 is not one of", [view(3)], [p8[:3]], [None], -1)
    # indexed16, and the palette
    refused(r"ImageUnpack: INDEXED takes one 8-bit index a pixel and gives 8-bit planes, not an index width of 16 \(indexed16 is not served\)", [view(2)], [p16[:3]], [p16[3]], iu.INDEXED, 16, pal)
    refused(r"ImageUnpack: INDEXED takes one 8-bit index a pixel .* not an index width of 4 ", [view(1)], [p8[:3]], [p8[3]], iu.INDEXED, 4, pal)
    refused("ImageUnpack: INDEXED needs a palette", [view(1)], [p8[:3]], [p8[3]], iu.INDEXED)
    refused("ImageUnpack: palette must be NULL for RGB", [view(3)], [p8[:3]], [None], iu.RGB, 8, pal)
    # per frame, naming it
    null = dev.wrap(0, h, w, 32, np.uint8)
    for k in range(3):
        planes = [null if j == k else p8[j] for j in range(3)]
        refused(r"ImageUnpack: frame 1: src, p\[0\], p\[1\] and p\[2\] must not be NULL", [view(3), view(3)], [p8[:3], planes], [None, None], iu.RGB)
    refused(r"ImageUnpack: frame 1: src, p\[0\], p\[1\] and p\[2\] must not be NULL", [view(4), dev.wrap(0, h, w * 4, w * 4, np.uint8)], [p8[:3], p8[:3]], [p8[3], p8[3]], iu.RGBA)
    refused(r"ImageUnpack: frame 0: src and p\[0\] must not be NULL", [view(2)], [[null]], [p8[3]], iu.GRAY_ALPHA)
    short = lambda p: dev.wrap(p.ptr, h, w, w - 1, p.dtype)
    geometry = r"ImageUnpack: frame 0: bad geometry 20x6, source pitch \d+ bytes for rows of \d+, plane pitches \d+ \.\. \d+"
    for k in range(3):
        refused(geometry, [view(3)], [[short(p8[j]) if j == k else p8[j] for j in range(3)]], [None], iu.RGB)
    refused(geometry, [view(4)], [p8[:3]], [short(p8[3])], iu.RGBA)
    refused(r"ImageUnpack: frame 0: bad geometry 20x6, source pitch 59 bytes for rows of 60", [dev.wrap(src.ptr, h, w * 3, w * 3 - 1, np.uint8)], [p8[:3]], [None], iu.RGB)
    refused(r"ImageUnpack: frame 0: bad geometry 20x6, source pitch 100 bytes for rows of 120", [dev.wrap(src.ptr, h, w * 6, 100, np.uint8)], [p16[:3]], [None], iu.RGB)
    for hh, ww in ((0, w), (h, 0), (-1, w)):
        refused("ImageUnpack: frame 0: bad geometry", [view(1)], [[dev.wrap(p8[0].ptr, hh, ww, 32, np.uint8)]], [None], iu.GRAY)  # (a frame's size is its first plane's)
    with pytest.raises(ValueError, match="one sample type"):
        dev.image_unpack([view(3)], [[p8[0], p16[1], p8[2]]], [None], iu.RGB)
    with pytest.raises(ValueError, match=r"palette is a C-contiguous \(256, 4\) uint8 array"):
        dev.image_unpack([view(1)], [p8[:3]], [p8[3]], iu.INDEXED, 8, np.zeros((3, 256), np.uint8))
    for p in p8 + p16:
        assert (dev.download(p) == 7).all()  # nothing was written by the refused calls
    dev.image_unpack([view(3)], [p8[:3]], [None], iu.RGB)  # and the valid call goes through
    assert all((dev.download(p) == 0).all() for p in p8[:3]) and (dev.download(p8[3]) == 7).all()
