#!/usr/bin/env python3
"""vszip_compress rates at 1080p (64 frames a call) and 4K (16) for YUV420P8 (all planes, chroma with the chroma tables) and GRAY8,
at mpeg2 qscale 8 and jpeg quality 50, beside two yardsticks on the very same planes: the 8-bit vszip_limiter (the streaming bound:
one byte read and one written a sample) and vszip_mosquito_nr u8 radius 1 restore 0 (the nearest fused integer kernel),
alternating call by call in one process.

fps, frac (the project's definition: algorithmic bytes / kernel time / 8.0 TB/s; 2 B/px for all three: a sample read, a sample
written) and the ratios `of Limiter` and `of MosquitoNR` (the yardstick's kernel time over the row's). Kernel time = the probe
around the call's launches, summed.

    python tools/compress_timing.py [--steps N]          (3 warm-up calls, then N >= 20 timed calls of every row)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import fixtures as fx  # noqa: E402
import vszip_amd  # noqa: E402
from vszip_amd import capi  # noqa: E402

PEAK = 8.0e12
SIZES = [("1080p", (1080, 1920), 64), ("4K", (2160, 3840), 16)]
# name, plane shapes of a frame relative to (h, w)
CLIPS = [("YUV420P8 all planes", [(1, 1), (2, 2), (2, 2)]), ("GRAY8", [(1, 1)])]


def plane(shape, k):
    """natural content with noise of a sixteenth: blocks with coefficients on both sides of the deadzone"""
    return (fx.tiled_natural(shape, np.uint8, k % 3) // 16 * 15 + (fx.splitmix64_plane(k, shape, np.uint8) >> 4)).astype(np.uint8)


def main():
    steps = max(20, int(sys.argv[sys.argv.index("--steps") + 1])) if "--steps" in sys.argv else 20
    d = vszip_amd.Device(0)
    for size, (h, w), nf in SIZES:
        for clip, rel in CLIPS:
            host = [[plane((h // a, w // b), 3 * fr + p) for p, (a, b) in enumerate(rel)] for fr in range(4)]
            srcs = [d.upload(p) for fr in range(nf) for p in host[fr % 4]]
            dsts = [d.empty(s.h, s.w, np.uint8) for s in srcs]
            n = len(srcs)
            px = sum(s.w * s.h for s in srcs)
            chroma = [i % len(rel) > 0 for i in range(n)]
            rows = [("Limiter u8 (1 in, 1 out)", d.prepared_limiter(srcs, dsts, [16.0] * n, [235.0] * n)),
                    ("MosquitoNR u8 radius 1 restore 0", d.prepared_mosquito_nr(srcs, dsts, 16, 0, 1, chroma=chroma)),
                    ("Compress mpeg2 qscale 8", d.prepared_compress(srcs, dsts, capi.compress_tables(0, qscale=8), chroma)),
                    ("Compress jpeg quality 50", d.prepared_compress(srcs, dsts, capi.compress_tables(1, quality=50), chroma))]
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
                    assert got >= 1, got
                    kern[k].append(ms)
            d.probe_enable(False)
            med = [float(np.median(k)) for k in kern]
            print(f"# {size} {clip} x{nf}: {n} planes, {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = median of the summed probe", flush=True)
            print(f"{'row':36s} {'B/px':>4s} {'kern ms':>8s} {'min ms':>8s} {'max ms':>8s} {'fps':>9s} {'TB/s':>6s} {'frac':>6s} {'of Limiter':>10s} {'of MosquitoNR':>13s}")
            for k, (name, _) in enumerate(rows):
                frac = 2 * px / (med[k] * 1e-3) / PEAK
                print(f"{name:36s} {2:4d} {med[k]:8.3f} {min(kern[k]):8.3f} {max(kern[k]):8.3f} {nf / (med[k] * 1e-3):9.0f} {frac * PEAK / 1e12:6.2f} {frac:6.3f} {med[0] / med[k]:10.2f} "
                      f"{med[1] / med[k]:13.2f}", flush=True)
            print(flush=True)
            for s in srcs + dsts:
                s.free()
    d.close()


if __name__ == "__main__":
    main()
