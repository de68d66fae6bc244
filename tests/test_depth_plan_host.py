"""The schedule of the error-diffusion kernel (vapoursynth-zip_amd/csrc/depth_plan.hpp, plain C++) on the host: tests/depth_plan_check.cpp is a
stand-alone program built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run directly; nothing is loaded into
Python. It replays the schedule as the kernel walks it for w in {1, 2, 3, 63, 64, 65, 129, 300} x h in {1, 2, 63, 64, 65, 129, 257, 1030} and both
workgroup sizes the kernel is built for (and a few wide planes: bands that wait for their wave, a carry row that leaves LDS): every sample computed
exactly once, every error read is the one the recurrence names and was written at an earlier step of the same wave or before an earlier barrier of
another, no seam slot overwritten before its last read, the same barrier count in every wave, and the bits of the serial restatement. The same
program prints the size and field offsets of vszip_depth_plane as the C compiler lays it out; they are compared with the ctypes class here."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not Path(probe).is_absolute():
        pytest.skip("g++ has no libasan")
    exe = tmp_path_factory.mktemp("depth_plan") / "depth_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + str(ROOT / "vapoursynth-zip_amd" / "csrc"), str(ROOT / "tests" / "depth_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    return r.returncode, r.stdout


def test_depth_plan_under_asan_ubsan(check_output):
    rc, out = check_output
    assert rc == 0 and " 0 failures" in out, out[-4000:]
    m = re.search(r"(\d+) plans swept, (\d+) samples", out)
    assert m and int(m.group(1)) >= 8 * 8 * 2 and int(m.group(2)) >= 2 * sum(w * h for w in (1, 2, 3, 63, 64, 65, 129, 300) for h in (1, 2, 63, 64, 65, 129, 257, 1030)), out[-2000:]


def test_ctypes_struct_has_the_compilers_layout(check_output):
    from vszip_amd import capi

    _, out = check_output
    seen = {}
    for line in out.splitlines():
        if line.startswith("struct "):
            t = line.split()
            seen[t[1]] = (int(t[3]), {t[i]: int(t[i + 1]) for i in range(4, len(t), 2)})
    assert set(seen) == set(capi.DEPTH_STRUCTS), set(seen) ^ set(capi.DEPTH_STRUCTS)
    header = (ROOT / "include" / "vszip_hip.h").read_text()
    assert set(re.findall(r"typedef struct (vszip_depth\w*)", header)) == set(seen)  # no struct of the entry point is left out
    for name, cls in capi.DEPTH_STRUCTS.items():
        size, offsets = seen[name]
        assert C.sizeof(cls) == size, (name, C.sizeof(cls), size)
        assert {f[0]: getattr(cls, f[0]).offset for f in cls._fields_} == offsets, name


def test_the_kernel_and_the_check_read_one_schedule():
    """depth.hip takes every scheduling decision from depth_plan.hpp: it defines no lag, ring size or chunk length of its own"""
    src = (ROOT / "vapoursynth-zip_amd" / "csrc" / "depth.hip").read_text()
    for name in ("make_plan", "slot_of", "column_of", "seam_column", "ring_slot", "has_carry", "carry_in_scratch", "diffuse", "kChunk", "kRing", "kCarryLds"):
        assert "dp::" + name in src, name
    assert not re.search(r"constexpr int k(Lag|Ring|Chunk|Skew)\w*\s*=", src)
