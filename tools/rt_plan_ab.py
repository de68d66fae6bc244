#!/usr/bin/env python3
"""One side of an A/B of the RT BoxBlur's host code (profiles/rt_plan.md): bench.py's RT legs, and the host time of 2000 queued one-frame calls
(1080p YUV420P8, 1 x 2 + 1 x 2 passes, no sync inside the loop: the plugin's case, where the planning is paid per call). One JSON line;
run it alternately with the library under test and the one it is compared with in vapoursynth-zip_amd/."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: F401,E402

import bench  # noqa: E402
import vszip_amd  # noqa: E402

dev = vszip_amd.Device(0)
timed = bench.Timed(dev, dev.sync, prewarm_s=0.3)  # as bench.py's main does
out = {}
for name in ("boxblur_rt_r30_4k", "boxblur_rt_r5x3_4k", "boxblur_rt_float_r5x3_4k"):
    out[name] = round(bench.boxblur_other_paths_leg(dev, timed, only=name)[name]["value"], 1)
out["boxblur_1080p_r1x2_yuv420p8"] = round(bench.boxblur_gauss_leg(dev, timed)["value"], 1)
out["boxblur_1080p_5pass"] = round(bench.boxblur_1080p_5pass_leg(dev, timed, True)["value"], 1)

shapes = bench.yuv420_shapes(1920, 1080)
srcs = [dev.empty(h, w, np.uint8) for h, w in shapes]
dsts = [dev.empty(h, w, np.uint8) for h, w in shapes]
table = dev.plane_table(srcs, dsts)
for _ in range(200):
    dev.boxblur_table(np.uint8, table, 1, 2, 1, 2)
dev.sync()
t0 = time.perf_counter()
for _ in range(2000):
    dev.boxblur_table(np.uint8, table, 1, 2, 1, 2)
t1 = time.perf_counter()
dev.sync()
t2 = time.perf_counter()
out["host_us_per_queued_call"] = round((t1 - t0) / 2000 * 1e6, 2)
out["us_per_call_with_drain"] = round((t2 - t0) / 2000 * 1e6, 2)
print(json.dumps(out), flush=True)
dev.close()
