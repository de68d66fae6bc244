#!/usr/bin/env python3
"""The recorded launch schedules of the RT BoxBlur (tests/rt_schedules.json): a fixed list of dev.boxblur calls and what each one launches.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/rt_schedule_calls.py run      (GPU: one process, nothing else traced)
    python3 tools/rt_schedule_calls.py collect DIR tests/rt_schedules.json                                (no GPU: trace -> JSON)
    python3 tools/rt_schedule_calls.py list                                                               (no GPU: the calls)

`run` issues the calls one by one, each behind a tiny Limiter call (its kernel is the separator in the trace) and a sync. `collect` cuts the
kernel trace at the separators and writes per call the sequence of [kernel, grid size in threads, workgroup size, LDS bytes] (the trace's
LDS_Block_Size: the kernel's static LDS; what a launch adds dynamically is not in it). The file is
compared with what rt_plan.hpp plans by tests/rt_plan_check.cpp: a change of routing has to re-record it on purpose, with this tool.

The calls: the benchmark's RT shapes, the same at one frame a call (what the plugin submits), every (shapes, args) of
test_rt_small_radius_multipass_kernels and test_rt_integer_chain_in_bands for u8 and u16 (the latter also under VSZIP_RT_ICHAIN_ALL, as
the test runs them), float planes up to seven passes an axis, and planes offset by one sample (nothing aligned). Plane contents do not
matter to the routing and are left as allocated."""
import csv
import glob
import json
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
ITEMSIZE = {"u8": 1, "u16": 2, "f16": 2, "f32": 4}
ALIGN_ELEMS = 32  # Device.empty's row pitch: whole groups of 32 samples


def yuv420(h, w):
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


SMALL = [([(72, 208), (36, 104), (36, 104)], (1, 2, 1, 2)), ([(300, 333)], (2, 3, 2, 2)), ([(64, 4096)], (3, 4, 0, 0)), ([(700, 96)], (0, 0, 4, 2)),
         ([(135, 251), (67, 125)], (5, 2, 6, 2)), ([(533, 130)], (7, 3, 8, 2)), ([(40, 35), (35, 40)], (8, 2, 8, 2)), ([(290, 640)], (1, 4, 1, 2)),
         ([(19, 40)], (2, 2, 2, 2)), ([(1080, 520)], (2, 2, 3, 2)),
         ([(72, 300), (36, 150)], (13, 5, 13, 5)), ([(90, 257)], (16, 2, 9, 2)), ([(64, 333)], (11, 3, 0, 0)), ([(50, 35)], (9, 4, 1, 2)), ([(40, 4104)], (12, 2, 0, 0)),
         ([(200, 70)], (0, 0, 2, 3)), ([(333, 131)], (0, 0, 5, 3)), ([(64, 64)], (0, 0, 3, 4)), ([(96, 35)], (0, 0, 1, 5)), ([(130, 200), (65, 100)], (2, 2, 3, 7)),
         ([(62, 48)], (0, 0, 30, 2)), ([(150, 41)], (0, 0, 22, 3)), ([(28, 260)], (0, 0, 13, 2)), ([(300, 5)], (0, 0, 4, 6)), ([(45, 3)], (0, 0, 2, 3)), ([(1080, 36)], (0, 0, 13, 5))]
BANDS = [([(1080, 36)], (0, 0, 13, 5)), ([(541, 130), (270, 65), (270, 65)], (0, 0, 5, 3)), ([(400, 70)], (0, 0, 2, 3)), ([(385, 64)], (0, 0, 3, 4)),
         ([(257, 33)], (0, 0, 1, 5)), ([(900, 48)], (0, 0, 30, 2)), ([(700, 41)], (0, 0, 22, 3)), ([(513, 260)], (2, 2, 13, 2)), ([(640, 5)], (0, 0, 4, 6)),
         ([(300, 3)], (0, 0, 2, 7)), ([(1081, 20)], (1, 2, 13, 5)), ([(136, 50)], (0, 0, 9, 3)), ([(2160, 64), (1080, 32)], (0, 0, 5, 3)),
         ([(540, 64)], (0, 0, 13, 5)), ([(540, 72)], (0, 0, 13, 4)), ([(540, 96), (270, 48), (270, 48)], (13, 5, 13, 5)), ([(1080, 40), (540, 20)], (0, 0, 13, 5))]
FLOAT = [("f32", yuv420(270, 480), 1, (5, 3, 5, 3)), ("f32", yuv420(2160, 3840), 4, (5, 3, 5, 3)), ("f32", [(300, 333)], 1, (2, 6, 2, 6)), ("f32", [(200, 130)], 1, (3, 7, 0, 0)),
         ("f16", [(540, 960)], 1, (0, 0, 4, 7)), ("f16", yuv420(270, 480), 50, (1, 2, 1, 2)), ("f32", [(64, 70)], 1, (30, 2, 30, 2)), ("f32", [(300, 300)], 1, (40, 3, 40, 3)),
         ("f32", [(131, 35)], 1, (1, 5, 1, 5)), ("f16", [(35, 131), (20, 64)], 1, (2, 4, 8, 2)), ("f32", [(1080, 1920)], 1, (30, 1, 30, 1))]
OFFSET = [("u8", [(72, 208)], (1, 2, 1, 2)), ("u16", [(300, 333)], (2, 3, 2, 3)), ("f32", [(200, 130)], (2, 3, 2, 3)), ("u16", [(1080, 520)], (13, 1, 13, 5))]


def calls():
    out = []

    def add(name, dtype, shapes, frames, args, options=None, offset=0):
        out.append({"name": name, "dtype": dtype, "frames": frames, "shapes": [list(s) for s in shapes], "offset": offset, "args": list(args), "options": options or {}})

    for frames in (None, 1):
        add("bench 4K YUV420P16 r30", "u16", yuv420(2160, 3840), frames or 8, (30, 1, 30, 1))
        add("bench 4K YUV420P16 r5x3", "u16", yuv420(2160, 3840), frames or 8, (5, 3, 5, 3))
        add("bench 4K YUV420PS r5x3", "f32", yuv420(2160, 3840), frames or 64, (5, 3, 5, 3))
        add("bench 1080p YUV420P8 r1x2", "u8", yuv420(1080, 1920), frames or 64, (1, 2, 1, 2))
        add("bench 1080p YUV420P16 r13x5", "u16", yuv420(1080, 1920), frames or 32, (13, 5, 13, 5))
    for dtype in ("u8", "u16"):
        for shapes, args in SMALL:
            add("small radius multipass", dtype, shapes, 1, args)
        for shapes, args in BANDS:
            add("chain in bands", dtype, shapes, 1, args)
            add("chain in bands", dtype, shapes, 1, args, {"VSZIP_RT_ICHAIN_ALL": 1})
    for dtype, shapes, frames, args in FLOAT:
        add("float", dtype, shapes, frames, args)
    for dtype, shapes, args in OFFSET:
        add("offset by one sample", dtype, shapes, 1, args, offset=1)
    return out


def plane_rows(call):
    """[h, w, source pitch, destination pitch, low four bits of source pointer | pitch bytes, the same of the destination] per plane of one frame"""
    isz = ITEMSIZE[call["dtype"]]
    rows = []
    for h, w in call["shapes"]:
        stride = -(-(w + call["offset"]) // ALIGN_ELEMS) * ALIGN_ELEMS
        low = (call["offset"] * isz | stride * isz) & 15  # (allocations are 256-byte aligned)
        rows.append([h, w, stride, stride, low, low])
    return rows


def run():
    import numpy as np

    sys.path.insert(0, str(ROOT))
    import vszip_amd

    np_dtype = {"u8": np.uint8, "u16": np.uint16, "f16": np.float16, "f32": np.float32}
    dev = vszip_amd.Device(0)
    sep_s, sep_d = dev.empty(8, 64, np.uint8), dev.empty(8, 64, np.uint8)

    def separator():
        dev.limiter([sep_s], [sep_d], [0], [255])
        dev.sync()

    for call in calls():
        dt, off = np_dtype[call["dtype"]], call["offset"]
        keep, srcs, dsts = [], [], []
        for _ in range(call["frames"]):
            for h, w in call["shapes"]:
                for lst in (srcs, dsts):
                    p = dev.empty(h, w + off, dt)
                    assert p.ptr % 256 == 0
                    keep.append(p)
                    lst.append(dev.wrap(p.ptr + off * p.dtype.itemsize, h, w, p.stride, dt) if off else p)
        separator()
        with dev.options(**call["options"]):
            dev.boxblur(srcs, dsts, *call["args"])
            dev.sync()
        del srcs, dsts, keep
    separator()
    dev.close()
    print(f"{len(calls())} calls issued")


_TYPES = (("unsigned short", "u16"), ("unsigned char", "u8"), ("_Float16", "f16"), ("float", "f32"))


def short_name(name):
    half = False
    if name.startswith("_Z"):  # the trace leaves names with _Float16 (DF16_) mangled, and so do older c++filt: demangle them as float
        half = "DF16_" in name
        name = subprocess.run(["c++filt", name.replace("DF16_", "f")], capture_output=True, text=True).stdout.strip() or name
    name = re.sub(r"\s*\[clone[^\]]*\]|\.kd$", "", name).replace("void ", "").replace("(anonymous namespace)::", "")
    name, lt, targs = name.split("(")[0].strip().partition("<")
    for long, short in _TYPES:  # (in the template arguments only)
        targs = targs.replace(long, "f16" if half and long == "float" else short)
    return name + lt + targs


def collect(trace_dir, out_path):
    rows = []
    for f in glob.glob(str(Path(trace_dir) / "**" / "*kernel_trace.csv"), recursive=True):
        rows += [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["start_timestamp"]))
    segs, seen_sep = [], False
    for r in rows:
        name = short_name(r["kernel_name"])
        if name.startswith("limiter_kernel"):
            segs.append([])
            seen_sep = True
        elif seen_sep and not name.startswith("__amd_rocclr"):
            segs[-1].append([name, int(r["grid_size_x"]) * int(r["grid_size_y"]) * int(r["grid_size_z"]),
                             int(r["workgroup_size_x"]) * int(r["workgroup_size_y"]) * int(r["workgroup_size_z"]), int(r["lds_block_size"])])
    cs = calls()
    assert len(segs) == len(cs) + 1 and not segs[-1], (len(segs), len(cs))
    lines = []
    for call, seg in zip(cs, segs):
        assert seg, call
        rec = {"name": call["name"], "dtype": call["dtype"], "frames": call["frames"], "planes": plane_rows(call), "args": call["args"], "options": call["options"], "kernels": seg}
        lines.append("  " + json.dumps(rec, separators=(",", ":")))
    Path(out_path).write_text('{"calls":[\n' + ",\n".join(lines) + "\n]}\n")
    print(f"{len(cs)} calls, {sum(len(s) for s in segs)} launches -> {out_path}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "list"
    if mode == "run":
        run()
    elif mode == "collect":
        collect(sys.argv[2], sys.argv[3])
    else:
        for c in calls():
            print(c)
