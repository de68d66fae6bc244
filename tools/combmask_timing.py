#!/usr/bin/env python3
"""vszip_comb_mask / vszip_comb_mask_mt rates beside two streaming kernels with the same stream counts, on the same planes in
the same process, alternating call by call: vszip_adaptive_binarize (two 8-bit streams in, one out) and 8-bit vszip_limiter
(one in, one out).

fps and frac (the project's definition: algorithmic bytes / kernel time / 8.0 TB/s). Algorithmic bytes: src + prv + dst once
each for the variants with motion (3 B/px), src + dst for the others (2 B/px). Kernel time = the probe around the call's
launches (one per table). The yardstick of a comb variant is its comparator's rate scaled by R / (R + halo): R = the band a
wave produces (comb_mask.hip kBandRows), halo = the extra source rows it loads (4: metric 0, 2: metric 1 and CombMaskMT) -
what a band kernel that re-read its halo from memory could reach.

    python tools/combmask_timing.py [--steps N]          (3 warm-up calls, then N >= 20 timed calls of every row)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/combmask_timing.py --steps 5     (the same under the profiler)
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
BAND_ROWS = 16  # comb_mask.hip kBandRows

CLIPS = [("1080p YUV420P8 x64", (1080, 1920), 64), ("4K YUV420P8 x16", (2160, 3840), 16)]


def frame(shape, f):
    """Y, U, V of frame f: natural content, shifted a row per frame like the reference's temporal fixture, odd rows pushed apart"""
    h, w = shape
    planes = []
    for p, s in enumerate([(h, w), (h // 2, w // 2), (h // 2, w // 2)]):
        a = np.roll(fx.tiled_natural(s, np.uint8, p), (f, 7 * f), axis=(0, 1)).astype(np.int32)
        a[1::2] += 12
        planes.append(np.clip(a, 0, 255).astype(np.uint8))
    return planes


def main():
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 20
    d = vszip_amd.Device(0)
    for clip, shape, nf in CLIPS:
        host = [frame(shape, f) for f in range(5)]
        srcs = [d.upload(p) for f in range(nf) for p in host[1 + f % 4]]
        prvs = [d.upload(p) for f in range(nf) for p in host[f % 4]]  # buffers of their own: every stream is read once a call
        dsts = [d.empty(s.h, s.w, np.uint8) for s in srcs]
        n = len(srcs)
        px = sum(s.w * s.h for s in srcs)
        rows = [  # name, call, streams (bytes per pixel), halo rows (None: a comparator)
            ("AdaptiveBinarize (2 in, 1 out)", lambda: d.adaptive_binarize(srcs, prvs, dsts, 3), 3, None),
            ("Limiter u8 (1 in, 1 out)", d.prepared_limiter(srcs, dsts, [16.0] * n, [235.0] * n), 2, None),
            ("CombMask default", d.prepared_comb_mask(srcs, dsts, prvs), 3, 4),
            ("CombMask metric=1", d.prepared_comb_mask(srcs, dsts, prvs, metric=1), 3, 2),
            ("CombMask expand=0", d.prepared_comb_mask(srcs, dsts, prvs, expand=False), 3, 4),
            ("CombMask mthresh=0", d.prepared_comb_mask(srcs, dsts, None, mthresh=0), 2, 4),
            ("CombMask mthresh=0 expand=0", d.prepared_comb_mask(srcs, dsts, None, mthresh=0, expand=False), 2, 4),
            ("CombMask mthresh=0 metric=1", d.prepared_comb_mask(srcs, dsts, None, mthresh=0, metric=1), 2, 2),
            ("CombMaskMT thY 30/30", d.prepared_comb_mask_mt(srcs, dsts, 30, 30), 2, 2),
            ("CombMaskMT thY 10/90", d.prepared_comb_mask_mt(srcs, dsts, 10, 90), 2, 2),
        ]
        for _ in range(3):
            for _, call, _, _ in rows:
                call()
        d.sync()
        d.probe_enable(True)
        d.probe_read()
        kern = [[] for _ in rows]
        for _ in range(steps):  # alternating: one call of every row per step
            for k, (_, call, _, _) in enumerate(rows):
                call()
                ms, launches = d.probe_read()
                assert launches == 1, launches
                kern[k].append(ms)
        d.probe_enable(False)
        med = [float(np.median(k)) for k in kern]
        frac = [rows[k][2] * px / (med[k] * 1e-3) / PEAK for k in range(len(rows))]
        comparator = {3: frac[0], 2: frac[1]}
        print(f"# {clip}: {n} planes, {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = median of the probe", flush=True)
        print(f"{'row':32s} {'B/px':>4s} {'kern ms':>8s} {'min ms':>8s} {'fps':>9s} {'TB/s':>6s} {'frac':>6s} {'yardstick':>9s} {'of it':>6s}")
        for k, (name, _, bpp, halo) in enumerate(rows):
            line = f"{name:32s} {bpp:4d} {med[k]:8.3f} {min(kern[k]):8.3f} {nf / (med[k] * 1e-3):9.0f} {frac[k] * PEAK / 1e12:6.2f} {frac[k]:6.3f}"
            if halo is not None:
                y = comparator[bpp] * BAND_ROWS / (BAND_ROWS + halo)
                line += f" {y:9.3f} {frac[k] / y:6.2f}"
            print(line, flush=True)
        print(flush=True)
        for s in srcs + prvs + dsts:
            s.free()
    d.close()


if __name__ == "__main__":
    main()
