#!/usr/bin/env python3
"""vszip_checkmate rates, both instantiations (tthr2 == 0: three input streams, tthr2 > 0: five), in two forms, beside two
streaming kernels on the same planes in the same process, alternating call by call: 8-bit vszip_limiter (one stream in, one
out) and vszip_adaptive_binarize (two in, one out).

  distinct  every stream in a buffer of its own: the kernel reads 3 or 5 B/px and writes 1 (algorithmic bytes 4 or 6 B/px)
  clip      Device.checkmate_clip: the neighbours are the clip's other frames, so every frame is needed once and written
            once (algorithmic bytes 2 B/px); what the kernel reads three or five times has to come out of the caches

fps and frac (the project's definition: algorithmic bytes / kernel time / 8.0 TB/s). Kernel time = the probe around the
call's launches (one per table of 128 planes), summed. The yardstick of a distinct row is the Limiter's frac scaled by
R / (R + 4): R = the rows of a band (checkmate.hip kBandRows), 4 = the halo rows its two waves load besides - what a band
kernel that re-read its halo from memory could reach at the Limiter's rate per byte. A clip row is compared with its
distinct row: `x distinct` is the distinct form's kernel time over the clip form's.

    python tools/checkmate_timing.py [--steps N]          (3 warm-up calls, then N >= 20 timed calls of every row)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/checkmate_timing.py --steps 5     (the same under the profiler)
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
BAND_ROWS, HALO_ROWS = 32, 4  # checkmate.hip kBandRows; rows y0 - 2, y0 - 1, y1, y1 + 1
TABLE = 128  # checkmate.hip kCheckPlanes

CLIPS = [("1080p YUV420P8 x64", (1080, 1920), 64), ("4K YUV420P8 x16", (2160, 3840), 16)]


def frame(shape, f):
    """Y, U, V of frame f: natural content with a few levels of noise per frame (with tthr2 = 8 both branches are taken)"""
    h, w = shape
    planes = []
    for p, s in enumerate([(h, w), (h // 2, w // 2), (h // 2, w // 2)]):
        a = fx.tiled_natural(s, np.uint8, p).astype(np.int32) + fx.splitmix64_plane(10 * f + p, s, np.uint8).astype(np.int32) % 13 - 6
        planes.append(np.clip(a, 0, 255).astype(np.uint8))
    return planes


def main():
    steps = max(20, int(sys.argv[sys.argv.index("--steps") + 1])) if "--steps" in sys.argv else 20
    d = vszip_amd.Device(0)
    for clip, shape, nf in CLIPS:
        host = [frame(shape, f) for f in range(8)]
        up = lambda off: [[d.upload(p) for p in host[(f + off) % 8]] for f in range(nf)]
        frames = up(2)  # the clip; and, for the distinct form, buffers of their own with what the neighbouring frames hold
        p2f, p1f, n1f, n2f = up(0), up(1), up(3), up(4)
        dstf = [[d.empty(s.h, s.w, np.uint8) for s in fr] for fr in frames]
        flat = lambda ff: [p for fr in ff for p in fr]
        srcs, dsts = flat(frames), flat(dstf)
        n = len(srcs)
        px = sum(s.w * s.h for s in srcs)
        launches = -(-n // TABLE)
        rows = [  # name, call, algorithmic bytes per pixel, launches, kind
            ("Limiter u8 (1 in, 1 out)", d.prepared_limiter(srcs, dsts, [16.0] * n, [235.0] * n), 2, 1, "yard"),
            ("AdaptiveBinarize (2 in, 1 out)", lambda: d.adaptive_binarize(srcs, flat(p1f), dsts, 3), 3, 1, "yard"),
            ("Checkmate tthr2=0 distinct", d.prepared_checkmate(srcs, dsts, flat(p1f), flat(n1f)), 4, launches, "distinct"),
            ("Checkmate tthr2=8 distinct", d.prepared_checkmate(srcs, dsts, flat(p1f), flat(n1f), flat(p2f), flat(n2f), tthr2=8), 6, launches, "distinct"),
            ("Checkmate tthr2=0 clip", d.prepared_checkmate_clip(frames, dstf), 2, launches, 2),
            ("Checkmate tthr2=8 clip", d.prepared_checkmate_clip(frames, dstf, tthr2=8), 2, launches, 3),
        ]
        for _ in range(3):
            for _, call, _, _, _ in rows:
                call()
        d.sync()
        d.probe_enable(True)
        d.probe_read()
        kern = [[] for _ in rows]
        for _ in range(steps):  # alternating: one call of every row per step
            for k, (_, call, _, nl, _) in enumerate(rows):
                call()
                ms, got = d.probe_read()
                assert got == nl, (got, nl)
                kern[k].append(ms)
        d.probe_enable(False)
        med = [float(np.median(k)) for k in kern]
        frac = [rows[k][2] * px / (med[k] * 1e-3) / PEAK for k in range(len(rows))]
        print(f"# {clip}: {n} planes, {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = median of the probe", flush=True)
        print(f"{'row':32s} {'B/px':>4s} {'kern ms':>8s} {'min ms':>8s} {'fps':>9s} {'TB/s':>6s} {'frac':>6s} {'yardstick':>9s} {'of it':>6s} {'x distinct':>10s}")
        for k, (name, _, bpp, _, kind) in enumerate(rows):
            line = f"{name:32s} {bpp:4d} {med[k]:8.3f} {min(kern[k]):8.3f} {nf / (med[k] * 1e-3):9.0f} {frac[k] * PEAK / 1e12:6.2f} {frac[k]:6.3f}"
            if kind == "distinct":
                y = frac[0] * BAND_ROWS / (BAND_ROWS + HALO_ROWS)
                line += f" {y:9.3f} {frac[k] / y:6.2f}"
            elif kind != "yard":
                line += f" {'':9s} {'':6s} {med[kind] / med[k]:10.2f}"
            print(line, flush=True)
        print(flush=True)
        for s in srcs + dsts + flat(p2f) + flat(p1f) + flat(n1f) + flat(n2f):
            s.free()
    d.close()


if __name__ == "__main__":
    main()
