#!/usr/bin/env python3
"""vszip_image_unpack rates at 1080p (64 frames a call) and 4K (16): rgb24, rgba32 with alpha, rgb48, rgba64, float32 and INDEXED on a
natural image and on noise (neighbouring pixels of an image hit the same palette entry, noise does not), beside the yardsticks on planes
of the same size in the same run: vszip_pack_rgb on RGB24, the mirror image, and vszip_limiter at each output sample width, alternating
call by call in one process. Sources are dense (the source pitch is the row's bytes, which the tool asserts), so an rgb24 row starts at
byte 3 w y; at both sizes that is a multiple of 16 for every format, so rgb24 is also run one pixel narrower, where row y starts 3 y
bytes before a multiple of 16: every phase from 0 to 15 occurs. Output planes are 16-byte aligned.

B/px is the algorithmic traffic (packed bytes read once, every plane byte written once; PackRGB 3 read and 4 written; Limiter 2, 4 or
8); TB/s = B/px x pixels / kernel time; frac = TB/s / 8.0; `of PackRGB` and `of Limiter` = the row's TB/s over the yardstick's (the
Limiter row of the output's sample width), from the medians, with the range the run's own spread allows in brackets: the row's slowest
call over the yardstick's fastest, and the reverse. Kernel time = the probe around the call's launches, summed. Before anything is
timed, frame 0 of every row is compared with the numpy spec (tests/image_unpack_ref.py).

    python tools/image_unpack_timing.py [--steps N]          (3 warm-up calls, then N >= 20 timed calls of every row)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import fixtures as fx  # noqa: E402
import image_unpack_ref as iu  # noqa: E402
import vszip_amd  # noqa: E402

PEAK = 8.0e12
SIZES = [("1080p", (1080, 1920), 64), ("4K", (2160, 3840), 16)]


def natural(h, w, dt, c, fr):
    """channel c of frame fr: the crop tiled, four different frames"""
    a = np.roll(fx.tiled_natural((h, w), np.uint8 if dt == np.float32 else dt, c % 3), 37 * fr, axis=1)
    return (a.astype(np.float32) / np.float32(255)) if dt == np.float32 else a


def make_rows(d, h, w, nf):
    """-> (rows, buffers): rows of (name, B/px, index of its Limiter row, its pixels as a fraction of h x w, call)"""
    bufs = []

    def keep(planes):
        bufs.append(planes)
        return planes
    up = lambda arrays: keep([d.upload(arrays[fr % len(arrays)]) for fr in range(nf)])
    out = lambda dt, n: [keep([d.empty(h, w, dt) for _ in range(nf)]) for _ in range(n)]
    o8, o16, o32 = out(np.uint8, 4), out(np.uint16, 4), out(np.float32, 4)
    nat = {dt: [[natural(h, w, dt, c, fr) for fr in range(4)] for c in range(4)] for dt in (np.uint8, np.uint16, np.float32)}
    r8, g8, b8 = (up(nat[np.uint8][c]) for c in range(3))
    l16, l32 = up(nat[np.uint16][0]), up(nat[np.float32][0])
    packed32 = keep([d.empty(h, w, np.uint32) for _ in range(nf)])
    rows = [("Limiter u8 (1 in, 1 out)", 2, 0, 1.0, d.prepared_limiter(r8, o8[0], [16.0] * nf, [235.0] * nf)),
            ("Limiter u16 (1 in, 1 out)", 4, 1, 1.0, d.prepared_limiter(l16, o16[0], [4096.0] * nf, [60160.0] * nf)),
            ("Limiter f32 (1 in, 1 out)", 8, 2, 1.0, d.prepared_limiter(l32, o32[0], [0.0] * nf, [1.0] * nf)),
            ("PackRGB RGB24 (3 in, 1 out)", 7, 0, 1.0, d.prepared_pack_rgb(r8, g8, b8, packed32, 8))]

    def unpack_row(name, layout, dt, planes_of, content4, pal=None):
        """content4: four (h, w', channels) arrays, w' <= w; the first is checked against the spec"""
        c, wc = iu.CHANNELS[layout], content4[0].shape[1]
        view = lambda p: p if wc == w else d.wrap(p.ptr, h, wc, p.stride, p.dtype)
        pxb = c * np.dtype(dt).itemsize
        packed = [iu.row_bytes(a) for a in content4]
        srcs = keep([d.upload(packed[fr % 4], align_elems=1) for fr in range(nf)])  # dense: the pitch is the row's bytes, whatever they are
        assert srcs[0].stride == wc * pxb and (srcs[0].stride % 16 != 0) == (wc != w), (name, srcs[0].stride)
        ncol = 1 if layout in (iu.GRAY, iu.GRAY_ALPHA) else 3
        planes = [[view(planes_of[k][fr]) for k in range(ncol)] for fr in range(nf)]
        alphas = [view(planes_of[ncol][fr]) if iu.HAS_ALPHA[layout] else None for fr in range(nf)]
        call = d.prepared_image_unpack(srcs, planes, alphas, layout, None, pal)
        call()
        d.sync()
        wp, wa = iu.unpack(content4[0], layout, None, pal)
        for got, want in zip(planes[0] + ([alphas[0]] if alphas[0] is not None else []), wp + ([wa] if wa is not None else [])):
            assert np.array_equal(iu.bits_of(d.download(got)), iu.bits_of(want)), name
        nout = ncol + (1 if iu.HAS_ALPHA[layout] else 0)
        rows.append((name, pxb + nout * (pxb // c if layout != iu.INDEXED else 1), {1: 0, 2: 1, 4: 2}[np.dtype(dt).itemsize], wc / w, call))

    inter = lambda dt, c: [np.ascontiguousarray(np.stack([nat[dt][k][fr] for k in range(c)], axis=2)) for fr in range(4)]
    for name, layout, dt, planes_of in (("rgb24 (1 in, 3 out)", iu.RGB, np.uint8, o8), ("rgba32 (1 in, 4 out)", iu.RGBA, np.uint8, o8), ("rgb48 (1 in, 3 out)", iu.RGB, np.uint16, o16),
                                        ("rgba64 (1 in, 4 out)", iu.RGBA, np.uint16, o16), ("float32 (1 in, 4 out)", iu.RGBA, np.float32, o32)):
        content4 = inter(dt, iu.CHANNELS[layout])
        unpack_row("Unpack " + name, layout, dt, planes_of, content4)
        if name.startswith("rgb24"):  # one pixel narrower: dense row y then starts 3 y bytes before a multiple of 16
            unpack_row("Unpack rgb24, w - 1: rows at odd bytes", layout, dt, planes_of, [np.ascontiguousarray(a[:, :-1]) for a in content4])
    pal = iu.palette(0)
    unpack_row("Unpack INDEXED natural (1 in, 4 out)", iu.INDEXED, np.uint8, o8, [nat[np.uint8][0][fr][:, :, None] for fr in range(4)], pal)
    unpack_row("Unpack INDEXED noise (1 in, 4 out)", iu.INDEXED, np.uint8, o8, [fx.splitmix64_plane(fr, (h, w), np.uint8)[:, :, None] for fr in range(4)], pal)
    return rows, bufs


def measure(d, rows, steps):
    """-> per row the kernel ms of `steps` calls, the rows alternating call by call, after 3 warm-up calls of each"""
    for _ in range(3):
        for row in rows:
            row[-1]()
    d.sync()
    d.probe_enable(True)
    d.probe_read()
    kern = [[] for _ in rows]
    for _ in range(steps):
        for k, row in enumerate(rows):
            row[-1]()
            ms, got = d.probe_read()
            assert got >= 1, got
            kern[k].append(ms)
    d.probe_enable(False)
    return kern


def report(size, nf, px, rows, kern, steps):
    med = [float(np.median(k)) for k in kern]
    rate = lambda k, ms: rows[k][1] * rows[k][3] * px / (ms * 1e-3) / 1e12
    pack = next(k for k, r in enumerate(rows) if r[0].startswith("PackRGB"))

    def ratio(k, y):
        return f"{rate(k, med[k]) / rate(y, med[y]):5.2f} [{rate(k, max(kern[k])) / rate(y, min(kern[y])):4.2f}, {rate(k, min(kern[k])) / rate(y, max(kern[y])):4.2f}]"
    print(f"# {size} x{nf}: {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = median of the summed probe", flush=True)
    print(f"{'row':38s} {'B/px':>4s} {'kern ms':>8s} {'min ms':>8s} {'max ms':>8s} {'fps':>9s} {'TB/s':>6s} {'frac':>6s} {'of PackRGB':>18s} {'of Limiter':>18s}")
    for k, (name, bpp, yard, _, _) in enumerate(rows):
        print(f"{name:38s} {bpp:4d} {med[k]:8.3f} {min(kern[k]):8.3f} {max(kern[k]):8.3f} {nf / (med[k] * 1e-3):9.0f} {rate(k, med[k]):6.2f} {rate(k, med[k]) * 1e12 / PEAK:6.3f} "
              f"{ratio(k, pack):>18s} {ratio(k, yard):>18s}", flush=True)
    print(flush=True)


def main():
    steps = max(20, int(sys.argv[sys.argv.index("--steps") + 1])) if "--steps" in sys.argv else 20
    d = vszip_amd.Device(0)
    for size, (h, w), nf in SIZES:
        rows, bufs = make_rows(d, h, w, nf)
        report(size, nf, h * w * nf, rows, measure(d, rows, steps), steps)
        for group in bufs:
            for p in group:
                p.free()
    d.close()


if __name__ == "__main__":
    main()
