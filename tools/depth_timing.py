#!/usr/bin/env python3
"""vszip_depth and vszip_deband_lowbit on YUV420P8 frames: 1080p x 64, 4K x 16 and one frame of each alone. Rows, alternating call by call
in one process: the up-conversion 8 -> 16 (dither none), the error-diffusion down-conversion 16 -> 8, vszip_deband sample mode 2 (range
15, with grain, the LDS tile path the default takes) on the same planes at 16 bits, and vszip_deband_lowbit whole (the three together on
the context's scratch).

Kernel time = the probe around the call's launches, summed (a call of more than 128 planes is several launches; the low-bit entry is the
conversions' and Deband's launches together). `of Deband` is the row's kernel time over that of the 16-bit Deband call beside it: the
down-conversion's share is the figure DESIGN.md 3.18 quotes. Mpx/s counts the samples of all planes.

    python tools/depth_timing.py [--steps N]          (3 warm-up calls, then N >= 10 timed calls of every row)

--fmt: the table of vszip_depth_fmt instead (profiles/depth_fmt_timing.txt), at 1080p x 64 and 4K x 16: u8 -> f32, u16 -> f32,
f32 -> u8 none, f32 -> f16 and f32 -> u8 error diffusion beside the 8 -> 16 none and 16 -> 8 error-diffusion rows of vszip_depth, in the same run,
alternating call by call. Streaming rows also as bytes moved (every sample read once and written once) over kernel time: median, the spread
min..max over the timed calls, and the median as a fraction of 8.0 TB/s.
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

SIZES = [("1080p", (1080, 1920), 64), ("4K", (2160, 3840), 16), ("1080p", (1080, 1920), 1), ("4K", (2160, 3840), 1)]
REL = [(1, 1), (2, 2), (2, 2)]  # YUV420


def plane8(shape, k):
    return (fx.tiled_natural(shape, np.uint8, k % 3) // 2 + (fx.splitmix64_plane(k, shape, np.uint8) >> 6) + 30).astype(np.uint8)


HBM_TBS = 8.0


def fmt_table(d, size, h, w, nf, steps):
    U8, U16, F16, F32 = (capi.U8, 8), (capi.U16, 16), (capi.F16, 16), (capi.F32, 32)
    host = [[plane8((h // a, w // b), 3 * fr + p) for p, (a, b) in enumerate(REL)] for fr in range(min(nf, 4))]
    src8 = [d.upload(p) for fr in range(nf) for p in host[fr % len(host)]]
    n, px = len(src8), sum(s.w * s.h for s in src8)
    chroma = [i % 3 > 0 for i in range(n)]
    dst8, a16, f32, h16 = ([d.empty(s.h, s.w, t) for s in src8] for t in (np.uint8, np.uint16, np.float32, np.float16))
    # (name, bytes a sample or 0 for the wavefront rows, call)
    rows = [("Depth 8 -> 16, none", 3, d.prepared_depth(src8, a16, 8, 16, capi.DITHER_NONE)),
            ("Depth 16 -> 8, error diffusion", 0, d.prepared_depth(a16, dst8, 16, 8, capi.DITHER_ERROR_DIFFUSION)),
            ("DepthFmt u8 -> f32, none", 5, d.prepared_depth_fmt(src8, f32, *U8, *F32, capi.DITHER_NONE, False, chroma)),
            ("DepthFmt u16 -> f32, none", 6, d.prepared_depth_fmt(a16, f32, *U16, *F32, capi.DITHER_NONE, False, chroma)),
            ("DepthFmt f32 -> u8, none", 5, d.prepared_depth_fmt(f32, dst8, *F32, *U8, capi.DITHER_NONE, False, chroma)),
            ("DepthFmt f32 -> f16", 6, d.prepared_depth_fmt(f32, h16, *F32, *F16)),
            ("DepthFmt f32 -> u8, error diffusion", 0, d.prepared_depth_fmt(f32, dst8, *F32, *U8, capi.DITHER_ERROR_DIFFUSION, True))]
    rows[0][2]()  # the 16-bit and the float planes the other rows read
    rows[2][2]()
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
    print(f"# {size} YUV420P8 x{nf}: {n} planes, {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = the summed probe", flush=True)
    print(f"{'row':38s} {'med ms':>8s} {'min ms':>8s} {'max ms':>8s} {'Mpx/s':>9s} {'B/sample':>8s} {'TB/s':>6s} {'min..max TB/s':>14s} {'of 8.0':>7s} {'of row':>7s}")
    for k, (name, bps, _) in enumerate(rows):
        med, lo, hi = float(np.median(kern[k])), min(kern[k]), max(kern[k])
        base = float(np.median(kern[0 if bps else 1]))
        line = f"{name:38s} {med:8.3f} {lo:8.3f} {hi:8.3f} {px / 1e6 / (med * 1e-3):9.0f}"
        if bps:
            tbs = lambda ms: px * bps / (ms * 1e-3) / 1e12
            base_tbs = px * 3 / (base * 1e-3) / 1e12
            line += f" {bps:8d} {tbs(med):6.2f} {tbs(hi):6.2f}..{tbs(lo):<6.2f} {tbs(med) / HBM_TBS:7.2f} {tbs(med) / base_tbs:7.2f}"
        else:
            line += f" {'':8s} {'':6s} {'':14s} {'':7s} {med / base:7.2f}"
        print(line, flush=True)
    print("# of row: a streaming row's bytes/s over the 8 -> 16 none row's; an error-diffusion row's kernel time over the 16 -> 8 row's", flush=True)
    print(flush=True)
    for s in src8 + dst8 + a16 + f32 + h16:
        s.free()


def main():
    steps = max(10, int(sys.argv[sys.argv.index("--steps") + 1])) if "--steps" in sys.argv else 10
    d = vszip_amd.Device(0)
    if "--fmt" in sys.argv:
        for size, (h, w), nf in SIZES[:2]:
            fmt_table(d, size, h, w, nf, steps)
        d.close()
        return
    for size, (h, w), nf in SIZES:
        host = [[plane8((h // a, w // b), 3 * fr + p) for p, (a, b) in enumerate(REL)] for fr in range(min(nf, 4))]
        src8 = [d.upload(p) for fr in range(nf) for p in host[fr % len(host)]]
        dst8 = [d.empty(s.h, s.w, np.uint8) for s in src8]
        a16, b16 = ([d.empty(s.h, s.w, np.uint16) for s in src8] for _ in range(2))
        n, px = len(src8), sum(s.w * s.h for s in src8)
        thr = 48 * 257
        tab = capi.deband_tables(w, h, 1, 1, nf, 15, 2, 7, grain=(4112, 4112))
        dt = d.upload_deband_tables(tab)
        entries = []
        for i in range(n):
            c = i % 3 > 0
            gw = w >> 1 if c else w
            entries.append(d.deband_entry(dt["chroma" if c else "luma"], int(c), int(c), dt["grain_c" if c else "grain_y"], 0, -(-gw * 2 // 32) * 32 // 2, thr, thr, thr, 0, 65535))
        rows = [("Deband mode 2 at 16 bits", d.prepared_deband(a16, b16, entries, 2, True, 1.5, 0.15, tab["max_offset"])),
                ("Depth 8 -> 16, none", d.prepared_depth(src8, a16, 8, 16, capi.DITHER_NONE)),
                ("Depth 16 -> 8, error diffusion", d.prepared_depth(b16, dst8, 16, 8, capi.DITHER_ERROR_DIFFUSION)),
                ("DebandLowbit 8 bits, whole", d.prepared_deband_lowbit(src8, dst8, entries, 8, False, 2, True, 1.5, 0.15, tab["max_offset"]))]
        rows[1][1]()  # the 16-bit planes Deband and the down-conversion work on
        rows[0][1]()
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
        print(f"# {size} YUV420P8 x{nf}: {n} planes, {px / 1e6:.1f} Mpx a call; {steps} calls a row, alternating, after 3 warm-up calls; kernel ms = median of the summed probe",
              flush=True)
        print(f"{'row':34s} {'kern ms':>9s} {'min ms':>9s} {'fps':>9s} {'Mpx/s':>9s} {'of Deband':>10s}")
        for k, (name, _) in enumerate(rows):
            print(f"{name:34s} {med[k]:9.3f} {min(kern[k]):9.3f} {nf / (med[k] * 1e-3):9.1f} {px / 1e6 / (med[k] * 1e-3):9.0f} {med[k] / med[0]:10.2f}", flush=True)
        print(flush=True)
        for s in src8 + dst8 + a16 + b16:
            s.free()
        for k in ("luma", "chroma", "grain_y", "grain_c"):
            if dt[k] is not None:
                dt[k].free()
    d.close()


if __name__ == "__main__":
    main()
