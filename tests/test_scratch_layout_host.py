"""The scratch layouts (vapoursynth-zip_amd/csrc/scratch_layout.hpp, plain C++) on the host: tests/scratch_layout_check.cpp is a stand-alone
program built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer. It checks the layout type (regions sequential and
disjoint, offsets multiples of their alignment, bytes() the end of the last region or pad, empty regions take no space, nested layouts at
base + outer offset + inner offset) and compares the layouts of PlaneStats, EEDI3 and SSIMULACRA2 - every region offset and the total - with the
size and pointer formulas these filters wrote by hand before, over 1 ... 192 planes and heights 1 ... 2160 (PlaneStats), vertical and horizontal
calls with and without dh, sclips, masks and vcheck, line lengths around the 64-column blocks and the 8192 threshold, one to six mixed planes
(EEDI3), and sizes from 8 x 8 to 4K including 1924 x 1080, 1 / 2 / 9 pairs, the split flags and every count of kept planes (SSIMULACRA2)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_scratch_layout_under_asan_ubsan(tmp_path):
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not Path(probe).is_absolute():
        pytest.skip("g++ has no libasan")
    exe = tmp_path / "scratch_layout_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + str(ROOT / "vapoursynth-zip_amd" / "csrc"), str(ROOT / "tests" / "scratch_layout_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(r.stdout.split()[-4]) > 1000000, out[-2000:]  # "<n> checks, 0 failures": the sweeps ran
