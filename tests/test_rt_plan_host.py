"""The schedule planner of the RT BoxBlur (vapoursynth-zip_amd/csrc/rt_plan.hpp, plain C++) on the host: tests/rt_plan_check.cpp is a stand-alone
program built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer. It sweeps u8 / u16 / f16 / f32, one to three planes and
batches, radii 1 ... 128, 0 ... 7 passes an axis, aligned and offset planes and the shipped option combinations (spans sum to the pass counts,
horizontal steps first, only the last step writes the caller's planes, no step reads the scratch set it writes, chains of 2 ... 5 stages within
their LDS limit, at least two bands), and it derives from the plan the kernel launches of every call recorded in tests/rt_schedules.json
(tools/rt_schedule_calls.py under a kernel trace on the GPU): kernel and template arguments, grid, workgroup and LDS bytes of the chain, hsmall and
banded steps, count and axis of the per-pass steps. A change of routing fails here and has to re-record that file on purpose."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_rt_plan_under_asan_ubsan(tmp_path):
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not Path(probe).is_absolute():
        pytest.skip("g++ has no libasan")
    rec = json.loads((ROOT / "tests" / "rt_schedules.json").read_text())["calls"]
    lines = []
    for c in rec:
        lines.append("call %s %d %d %d %d %d %s" % (c["dtype"], c["frames"], *c["args"], c["name"]))
        lines += ["plane %d %d %d %d %d %d" % tuple(p) for p in c["planes"]]
        lines += ["opt %s %d" % kv for kv in sorted(c["options"].items())]
        lines += ["k %d %d %d %s" % (k[1], k[2], k[3], k[0]) for k in c["kernels"]]
    listing = tmp_path / "rt_schedules.txt"
    listing.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "rt_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + str(ROOT / "vapoursynth-zip_amd" / "csrc"), str(ROOT / "tests" / "rt_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe), str(listing)], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert "%d recorded calls" % len(rec) in r.stdout and len(rec) >= 100, out[-2000:]
