#!/usr/bin/env python3
"""vszip_deband rates at 1080p (64 frames a call) and 4K (16) for YUV420P16 (all planes, with grain) and GRAYS (with grain), in
sample modes 2 (the default) and 7, at ranges 15 and 31, with each gather path forced (VSZIP_DEBAND_PATH: 1 the LDS tile, 2 global
memory), beside vszip_limit_filter with a third clip on the very same planes (three streams in, one out, like Deband's source, table
and grain), alternating call by call in one process.

fps, frac (the project's definition: algorithmic bytes / kernel time / 8.0 TB/s; Deband's algorithmic bytes are the source, the
two-byte table entry, the grain and the destination: 8 B/px at 16 bits, 14 B/px for float; mode 7's angle plane is an intermediate
and is not counted) and `of LimitFilter` (the yardstick's kernel time over the row's). Kernel time = the probe around the call's
launches, summed (a call of more than 96 planes is several launches; mode 7 adds the angle kernel).

    python tools/deband_timing.py [--steps N]          (3 warm-up calls, then N >= 20 timed calls of every row)
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
# name, dtype, plane shapes of a frame relative to (h, w), chroma subsampling
CLIPS = [("YUV420P16 all planes", np.uint16, [(1, 1), (2, 2), (2, 2)], 1), ("GRAYS", np.float32, [(1, 1)], 0)]


def plane(shape, dtype, k):
    a = fx.tiled_natural(shape, dtype, k % 3)
    if np.dtype(dtype) == np.float32:
        return (a * np.float32(0.9) + fx.splitmix64_plane(k, shape, np.float32) * np.float32(0.02)).astype(np.float32)
    return (a // 2 + (fx.splitmix64_plane(k, shape, dtype) >> 6) + 8000).astype(dtype)


def main():
    steps = max(20, int(sys.argv[sys.argv.index("--steps") + 1])) if "--steps" in sys.argv else 20
    d = vszip_amd.Device(0)
    for size, (h, w), nf in SIZES:
        for clip, dtype, rel, ss in CLIPS:
            f = np.dtype(dtype) == np.float32
            isz = np.dtype(dtype).itemsize
            host = [[plane((h // a, w // b), dtype, 3 * fr + p) for p, (a, b) in enumerate(rel)] for fr in range(4)]
            srcs = [d.upload(p) for fr in range(nf) for p in host[fr % 4]]
            seconds = [d.upload(p) for fr in range(nf) for p in host[(fr + 1) % 4]]
            thirds = [d.upload(p) for fr in range(nf) for p in host[(fr + 2) % 4]]
            dsts = [d.empty(s.h, s.w, dtype) for s in srcs]
            n = len(srcs)
            px = sum(s.w * s.h for s in srcs)
            thr = 48 / 255.0 if f else 48 * 257
            rows = [("LimitFilter + third clip (3 in, 1 out)", 4 * isz, lambda: d.limit_filter(srcs, seconds, dsts, [thr] * n, [thr] * n, [2.0] * n, refs=thirds))]
            keep = []
            for mode in (2, 7):
                for rng in (15, 31):
                    tab = capi.deband_tables(w, h, ss, ss, nf, rng, mode, 7, grain=(16 / 255.0, 16 / 255.0) if f else (4112, 4112), is_float=f)
                    dt = d.upload_deband_tables(tab)
                    keep.append(dt)
                    entries = []
                    for i, s in enumerate(srcs):
                        c = len(rel) > 1 and i % len(rel) > 0
                        gw = w >> ss if c else w
                        entries.append(d.deband_entry(dt["chroma" if c else "luma"], ss if c else 0, ss if c else 0, dt["grain_c" if c else "grain_y"], 0,
                                                      -(-gw * isz // 32) * 32 // isz, thr, thr, thr, (-0.5 if c else 0.0) if f else 0, (0.5 if c else 1.0) if f else 65535))
                    call = d.prepared_deband(srcs, dsts, entries, mode, True, 1.5, 0.15, tab["max_offset"])
                    for path, pname in ((1, "tile"), (2, "direct")):
                        def run(call=call, path=path):
                            d.set_option("VSZIP_DEBAND_PATH", path)
                            call()
                        rows.append((f"Deband mode {mode} range {rng} {pname}", (8 if not f else 14), run))
            for _ in range(3):
                for _, _, call in rows:
                    call()
            d.sync()
            d.probe_enable(True)
            d.probe_read()
            kern = [[] for _ in rows]
            for _ in range(steps):  # alternating: one call of every row per step
                for k, (_, _, call) in enumerate(rows):
                    call()
                    ms, got = d.probe_read()
                    assert got >= 1, got
                    kern[k].append(ms)
            d.probe_enable(False)
            d.set_option("VSZIP_DEBAND_PATH", 0)
            med = [float(np.median(k)) for k in kern]
            print(f"# {size} {clip} x{nf}: {n} planes, {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = median of the summed probe", flush=True)
            print(f"{'row':40s} {'B/px':>4s} {'kern ms':>8s} {'min ms':>8s} {'fps':>9s} {'TB/s':>6s} {'frac':>6s} {'of LimitFilter':>14s}")
            for k, (name, bpp, _) in enumerate(rows):
                frac = bpp * px / (med[k] * 1e-3) / PEAK
                print(f"{name:40s} {bpp:4d} {med[k]:8.3f} {min(kern[k]):8.3f} {nf / (med[k] * 1e-3):9.0f} {frac * PEAK / 1e12:6.2f} {frac:6.3f} {med[0] / med[k]:14.2f}", flush=True)
            print(flush=True)
            for s in srcs + seconds + thirds + dsts:
                s.free()
            for dt in keep:
                for k in ("luma", "chroma", "grain_y", "grain_c"):
                    if dt[k] is not None:
                        dt[k].free()
    d.close()


if __name__ == "__main__":
    main()
