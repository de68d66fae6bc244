#!/usr/bin/env python3
"""vszip_clahe rates: fps and frac (the project's definition: every input byte read once and every output byte written once,
divided by the kernel time, divided by 8.0 TB/s). Kernel time = the probe around each plane group's three launches (histogram,
LUT, interpolation); `stream` is the whole region on the stream (also the histogram zeroing and the launch gaps).

    python tools/clahe_timing.py [--steps N]
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


def frame(shape, dtype, content, f):
    h, w = shape
    planes = []
    for p, s in enumerate([(h, w), (h // 2, w // 2), (h // 2, w // 2)]):
        if content == "natural":
            planes.append(np.ascontiguousarray(np.roll(fx.tiled_natural(s, dtype, p), 7 * f, axis=1)))
        elif content == "noise":
            planes.append(fx.splitmix64_plane(1000 * f + p, s, dtype))
        else:
            planes.append(np.full(s, 30000 if dtype == np.uint16 else 117, dtype))
    return planes


ROWS = [  # name, (h, w), dtype, frames a call, tiles, content
    ("4K YUV420P16 natural tiles=3", (2160, 3840), np.uint16, 16, 3, "natural"),
    ("4K YUV420P16 natural tiles=8", (2160, 3840), np.uint16, 16, 8, "natural"),
    ("4K YUV420P16 natural tiles=3, 1 frame", (2160, 3840), np.uint16, 1, 3, "natural"),
    ("1080p YUV420P8 natural tiles=3", (1080, 1920), np.uint8, 64, 3, "natural"),
    ("4K YUV420P16 flat tiles=3", (2160, 3840), np.uint16, 16, 3, "flat"),
    ("4K YUV420P16 noise tiles=3", (2160, 3840), np.uint16, 16, 3, "noise"),
    ("1080p YUV420P8 flat tiles=3", (1080, 1920), np.uint8, 64, 3, "flat"),
    ("1080p YUV420P8 noise tiles=3", (1080, 1920), np.uint8, 64, 3, "noise"),
]


def main():
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 20
    only = [a for a in sys.argv[1:] if a.isdigit() and a != str(steps)]
    d = vszip_amd.Device(0)
    print(f"{'row':42s} {'ms/call':>8s} {'kern ms':>8s} {'fps':>9s} {'frac':>6s} {'stream frac':>11s}", flush=True)
    for i, (name, shape, dtype, nf, tiles, content) in enumerate(ROWS):
        if only and str(i) not in only:
            continue
        host = [p for f in range(min(nf, 4)) for p in frame(shape, dtype, content, f)]
        srcs = [d.upload(host[k % len(host)]) for k in range(3 * nf)]
        dsts = [d.empty(s.h, s.w, dtype) for s in srcs]
        call = d.prepared_clahe(srcs, dsts, 7 if dtype == np.uint8 else 2560, tiles)
        for _ in range(3):
            call()
        d.sync()
        d.probe_enable(True)
        d.timer_start()
        for _ in range(steps):
            call()
        region = d.timer_stop_ms() / steps
        kern, _ = d.probe_read()
        kern /= steps
        d.probe_enable(False)
        nbytes = 2 * sum(s.w * s.h * s.dtype.itemsize for s in srcs)
        print(f"{name:42s} {region:8.3f} {kern:8.3f} {nf / (kern * 1e-3):9.0f} {nbytes / (kern * 1e-3) / PEAK:6.3f} {nbytes / (region * 1e-3) / PEAK:11.3f}",
              flush=True)
        for s in srcs + dsts:
            s.free()
    d.close()


if __name__ == "__main__":
    main()
