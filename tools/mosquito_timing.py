#!/usr/bin/env python3
"""vszip_mosquito_nr rates at 1080p and 4K for three clips - YUV420P8 with the luma processed (the wrapper's default
planes), YUV420P16 with all three planes processed, GRAYS - with radius 1 and 2 and restore 0 (the smoothing alone) and
128 (the wavelet exchange), beside vszip_limiter on the same planes in the same process, alternating call by call: the
Limiter reads every sample once and writes it once, which is all MosquitoNR has to move as well.

fps, frac (the project's definition: algorithmic bytes / kernel time / 8.0 TB/s, the algorithmic bytes being
2 x bytes per sample per pixel) and `of Limiter` (the Limiter's kernel time over the row's). Kernel time = the probe
around the call's launch.

    python tools/mosquito_timing.py [--steps N]          (3 warm-up calls, then N >= 20 timed calls of every row)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mosquito_timing.py --steps 5     (the same under the profiler)
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

SIZES = [("1080p", (1080, 1920), 32), ("4K", (2160, 3840), 8)]
# name, dtype, bits, plane shapes of a frame relative to (h, w) that are processed, Limiter bounds
CLIPS = [
    ("YUV420P8 luma", np.uint8, 8, [(1, 1)], (16.0, 235.0)),
    ("YUV420P16 all planes", np.uint16, 16, [(1, 1), (2, 2), (2, 2)], (4096.0, 60160.0)),
    ("GRAYS", np.float32, 32, [(1, 1)], (0.0, 1.0)),
]


def plane(shape, dtype, k):
    """natural content with a few levels of noise, so that directions vary and few samples are flat"""
    a = fx.tiled_natural(shape, dtype, k % 3)
    if np.dtype(dtype) == np.float32:
        return (a + (fx.splitmix64_plane(k, shape, np.float32) - np.float32(0.5)) * np.float32(0.02)).astype(np.float32)
    peak = np.iinfo(dtype).max
    amp = 5 if np.dtype(dtype) == np.uint8 else 1285
    n = fx.splitmix64_plane(k, shape, dtype).astype(np.int64) % amp - amp // 2
    return np.clip(a.astype(np.int64) + n, 0, peak).astype(dtype)


def main():
    steps = max(20, int(sys.argv[sys.argv.index("--steps") + 1])) if "--steps" in sys.argv else 20
    d = vszip_amd.Device(0)
    for size, (h, w), nf in SIZES:
        for clip, dtype, bits, rel, (lo, hi) in CLIPS:
            host = [[plane((h // a, w // b), dtype, 3 * f + p) for p, (a, b) in enumerate(rel)] for f in range(4)]
            srcs = [d.upload(p) for f in range(nf) for p in host[f % 4]]
            dsts = [d.empty(s.h, s.w, dtype) for s in srcs]
            n = len(srcs)
            px = sum(s.w * s.h for s in srcs)
            b = None if bits == 32 else bits
            rows = [("Limiter (1 in, 1 out)", d.prepared_limiter(srcs, dsts, [lo] * n, [hi] * n))]
            for radius in (1, 2):
                for restore in (0, 128):
                    rows.append((f"MosquitoNR radius={radius} restore={restore}", d.prepared_mosquito_nr(srcs, dsts, 16, restore, radius, b)))
            for _ in range(3):
                for _, call in rows:
                    call()
            d.sync()
            d.probe_enable(True)
            d.probe_read()
            kern = [[] for _ in rows]
            for _ in range(steps):  # alternating: one call of every row per step
                for k, (_, call) in enumerate(rows):
                    call()
                    ms, got = d.probe_read()
                    assert got == 1, got
                    kern[k].append(ms)
            d.probe_enable(False)
            med = [float(np.median(k)) for k in kern]
            bpp = 2 * np.dtype(dtype).itemsize
            print(f"# {size} {clip} x{nf}: {n} planes, {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = median of the probe", flush=True)
            print(f"{'row':34s} {'B/px':>4s} {'kern ms':>8s} {'min ms':>8s} {'fps':>9s} {'TB/s':>6s} {'frac':>6s} {'of Limiter':>10s}")
            for k, (name, _) in enumerate(rows):
                frac = bpp * px / (med[k] * 1e-3) / PEAK
                print(f"{name:34s} {bpp:4d} {med[k]:8.3f} {min(kern[k]):8.3f} {nf / (med[k] * 1e-3):9.0f} {frac * PEAK / 1e12:6.2f} {frac:6.3f} {med[0] / med[k]:10.2f}", flush=True)
            print(flush=True)
            for s in srcs + dsts:
                s.free()
    d.close()


if __name__ == "__main__":
    main()
