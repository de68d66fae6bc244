#!/usr/bin/env python3
"""vszip_bilateral_dither rates at 1080p (64 frames a call) and 4K (16) for YUV420P8 (all planes), YUV420P16 (all planes) and GRAYS:
the reference's default (radius 16, thr 2.5, flat 0.4, subspl 0: K = 30 sub-sampled taps) with and without a `ref` clip, the goldens'
dense radius 8 (225 taps) and dense radius 16 (961 taps), each on the tile path and on the direct path (VSZIP_BILATERAL_DITHER_PATH 1 / 2),
beside vszip_bilateral with its defaults and vszip_limiter on the very same planes, alternating call by call in one process.

fps, taps/s, frac (the project's definition: algorithmic bytes / kernel time / 8.0 TB/s; the algorithmic bytes are src + dst, plus ref
where one is given) and `vec` (taps/s x 5 operations against the 157.3 TFLOPS fp32 vector peak). Kernel time = the probe around the
call's launches, summed (a call is several launches: 96 table entries or 2^36 taps each at most).

    python tools/bilateral_dither_timing.py [--steps N]          (2 warm-up calls, then N >= 5 timed calls of every row)
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
VEC_PEAK = 157.3e12
OPS_PER_TAP = 5
SIZES = [("1080p", (1080, 1920), 64), ("4K", (2160, 3840), 16)]
CLIPS = [("YUV420P8 all planes", np.uint8, [(1, 1), (2, 2), (2, 2)]), ("YUV420P16 all planes", np.uint16, [(1, 1), (2, 2), (2, 2)]), ("GRAYS", np.float32, [(1, 1)])]
# name, radius, subspl, with ref
ROWS = [("default r16 subspl 0 (K 30)", 16, 0.0, False), ("default r16 subspl 0 + ref", 16, 0.0, True), ("dense r8 (225 taps)", 8, 2.0, False),
        ("dense r16 (961 taps)", 16, 2.0, False)]


def plane(shape, dtype, k):
    a, n = fx.tiled_natural(shape, dtype, k % 3), fx.splitmix64_plane(k, shape, dtype)
    if np.dtype(dtype) == np.float32:
        return (a * np.float32(0.5) + n * np.float32(0.06)).astype(np.float32)
    return (a // 2 + (n >> 4)).astype(dtype)


def main():
    steps = max(5, int(sys.argv[sys.argv.index("--steps") + 1])) if "--steps" in sys.argv else 10
    d = vszip_amd.Device(0)
    for size, (h, w), nf in SIZES:
        for clip, dtype, rel in CLIPS:
            f = np.dtype(dtype) == np.float32
            isz = np.dtype(dtype).itemsize
            bits = 32 if f else 8 * isz
            host = [[plane((h // a, w // b), dtype, 3 * fr + p) for p, (a, b) in enumerate(rel)] for fr in range(4)]
            srcs = [d.upload(p) for fr in range(nf) for p in host[fr % 4]]
            refs = [d.upload(p) for fr in range(nf) for p in host[(fr + 1) % 4]]
            dsts = [d.empty(s.h, s.w, dtype) for s in srcs]
            n = len(srcs)
            px = sum(s.w * s.h for s in srcs)
            cfg = d.bilateral_cfg(yuv=len(rel) > 1, ssw=int(len(rel) > 1), ssh=int(len(rel) > 1), hist_len=256 if isz == 1 else 65536)
            idx = [i % len(rel) for i in range(n)]
            lo, hi = [0.0] * n, [0.9 if f else float((1 << bits) - 2)] * n
            limiter = d.prepared_limiter(srcs, dsts, lo, hi)
            rows = [("Limiter (1 in, 1 out)", 2 * isz, 0, limiter), ("Bilateral, its defaults", 2 * isz, 0, lambda: d.bilateral(srcs, dsts, cfg, idx, peak=255.0 if isz == 1 else None))]
            keep = []
            for name, radius, subspl, with_ref in ROWS:
                p = capi.bilateral_dither_params(f, bits, radius, 8.0 if subspl == 2.0 else 2.5, 0.4, 0.0, subspl)
                pts = d.upload_bilateral_dither_points(capi.bilateral_dither_points(radius, subspl)) if p["subsampled"] else None
                keep.append(pts)
                e = [d.bilateral_dither_entry(radius, p["m"], p["wmax"], p["sum_w_min"], pts, p["K"])] * n
                call = d.prepared_bilateral_dither(srcs, dsts, e, refs if with_ref else None, bits)
                taps = p["K"] if p["subsampled"] else (2 * radius - 1) ** 2
                for path, pname in ((1, "tile"), (2, "direct")):
                    def run(call=call, path=path):
                        d.set_option("VSZIP_BILATERAL_DITHER_PATH", path)
                        call()
                    rows.append((f"{name} {pname}", (3 if with_ref else 2) * isz, taps, run))
            for _ in range(2):
                for _, _, _, call in rows:
                    call()
            d.sync()
            d.probe_enable(True)
            d.probe_read()
            kern = [[] for _ in rows]
            for _ in range(steps):  # alternating: one call of every row per step
                for k, (_, _, _, call) in enumerate(rows):
                    call()
                    ms, got = d.probe_read()
                    assert got >= 1, got
                    kern[k].append(ms)
            d.probe_enable(False)
            d.set_option("VSZIP_BILATERAL_DITHER_PATH", 0)
            med = [float(np.median(k)) for k in kern]
            print(f"# {size} {clip} x{nf}: {n} planes, {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 2 warm-up calls; kernel ms = median of the summed probe", flush=True)
            print(f"{'row':36s} {'B/px':>4s} {'kern ms':>9s} {'min ms':>9s} {'fps':>8s} {'Gtaps/s':>8s} {'frac':>6s} {'vec':>6s} {'of Bilateral':>12s} {'of Limiter':>10s}")
            for k, (name, bpp, taps, _) in enumerate(rows):
                t = med[k] * 1e-3
                rate = taps * px / t
                print(f"{name:36s} {bpp:4d} {med[k]:9.3f} {min(kern[k]):9.3f} {nf / t:8.0f} {rate / 1e9:8.1f} {bpp * px / t / PEAK:6.3f} {rate * OPS_PER_TAP / VEC_PEAK:6.3f} "
                      f"{med[1] / med[k]:12.3f} {med[0] / med[k]:10.4f}", flush=True)
            print(flush=True)
            for s in srcs + refs + dsts + [p for p in keep if p is not None]:
                s.free()
    d.close()


if __name__ == "__main__":
    main()
