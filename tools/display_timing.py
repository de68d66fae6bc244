#!/usr/bin/env python3
"""vszip_pack_rgb and vszip_color_map rates at 1080p (64 frames a call) and 4K (16): PackRGB on RGB24 and RGB30, ColorMap on a natural
image and on uniform noise (neighbouring samples of an image hit the same table entry, noise does not), beside the yardstick on planes
of the same size: vszip_limiter on 8-bit and on 16-bit planes, the existing streaming kernels (a sample read, a sample written),
alternating call by call in one process.

B/px is the algorithmic traffic (PackRGB 3 or 6 bytes read and 4 written; ColorMap 1 read and 3 written; Limiter 2 or 4); TB/s = B/px x
samples / kernel time; frac = TB/s / 8.0; `of Limiter` = the row's TB/s over the TB/s of the Limiter row of its sample width (RGB30: the
16-bit one). The margin of that comparison is the run's own spread: the min and max columns. Kernel time = the probe around the call's
launches, summed.

    python tools/display_timing.py [--steps N]          (3 warm-up calls, then N >= 20 timed calls of every row)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import fixtures as fx  # noqa: E402
import vszip_amd  # noqa: E402

PEAK = 8.0e12
SIZES = [("1080p", (1080, 1920), 64), ("4K", (2160, 3840), 16)]


def make_rows(d, h, w, nf):
    """-> (rows, buffers): rows of (name, B/px, index of its Limiter row, call)"""
    up = lambda planes: [d.upload(planes[fr % len(planes)]) for fr in range(nf)]
    nat8 = [[fx.tiled_natural((h, w), np.uint8, (fr + c) % 3) for fr in range(4)] for c in range(3)]
    for c in range(3):
        for fr in range(4):
            nat8[c][fr] = np.roll(nat8[c][fr], 37 * fr, axis=1)  # four different frames
    r8, g8, b8 = (up(nat8[c]) for c in range(3))
    r16, g16, b16 = (up([((p.astype(np.uint32) * 1023 + 127) // 255).astype(np.uint16) for p in nat8[c]]) for c in range(3))
    noise = up([fx.splitmix64_plane(fr, (h, w), np.uint8) for fr in range(4)])
    packed = [d.empty(h, w, np.uint32) for _ in range(nf)]
    o8 = [[d.empty(h, w, np.uint8) for _ in range(nf)] for _ in range(3)]
    o16 = [d.empty(h, w, np.uint16) for _ in range(nf)]
    lut = np.stack([np.random.default_rng(c).permutation(256) for c in range(3)]).astype(np.uint8)
    rows = [("Limiter u8 (1 in, 1 out)", 2, 0, d.prepared_limiter(r8, o8[0], [16.0] * nf, [235.0] * nf)),
            ("Limiter u16 (1 in, 1 out)", 4, 1, d.prepared_limiter(r16, o16, [64.0] * nf, [940.0] * nf)),
            ("PackRGB RGB24 (3 in, 1 out)", 7, 0, d.prepared_pack_rgb(r8, g8, b8, packed, 8)),
            ("PackRGB RGB30 (3 in, 1 out)", 10, 1, d.prepared_pack_rgb(r16, g16, b16, packed, 10)),
            ("ColorMap natural (1 in, 3 out)", 4, 0, d.prepared_color_map(r8, o8[0], o8[1], o8[2], lut)),
            ("ColorMap noise (1 in, 3 out)", 4, 0, d.prepared_color_map(noise, o8[0], o8[1], o8[2], lut))]
    return rows, [r8, g8, b8, r16, g16, b16, noise, packed, *o8, o16]


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
    tbs = [bpp * px / (m * 1e-3) / 1e12 for (_, bpp, _, _), m in zip(rows, med)]
    print(f"# {size} x{nf}: {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = median of the summed probe", flush=True)
    print(f"{'row':32s} {'B/px':>4s} {'kern ms':>8s} {'min ms':>8s} {'max ms':>8s} {'fps':>9s} {'TB/s':>6s} {'frac':>6s} {'of Limiter':>10s}")
    for k, (name, bpp, yard, _) in enumerate(rows):
        print(f"{name:32s} {bpp:4d} {med[k]:8.3f} {min(kern[k]):8.3f} {max(kern[k]):8.3f} {nf / (med[k] * 1e-3):9.0f} {tbs[k]:6.2f} {tbs[k] * 1e12 / PEAK:6.3f} "
              f"{tbs[k] / tbs[yard]:10.2f}", flush=True)
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
