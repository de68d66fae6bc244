"""The band planner of the BoxBlur ring kernel (vapoursynth-zip_amd/csrc/ring_bands.hpp, plain C++) on the host: tests/ring_bands_check.cpp is a
stand-alone program built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer. It sweeps heights 53 ... 2200, ring periods
4 ... 46 and band targets 1 ... 96 (bands tile the plane, each at least one period, row counts within one of each other) and plans the headline batch
(64 4K YUV420P16 frames, r = 13: 3072 bands of 540 rows)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_ring_bands_planner_under_asan_ubsan(tmp_path):
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not Path(probe).is_absolute():
        pytest.skip("g++ has no libasan")
    exe = tmp_path / "ring_bands_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + str(ROOT / "vapoursynth-zip_amd" / "csrc"), str(ROOT / "tests" / "ring_bands_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failures" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert "3072 bands of 540 rows" in r.stdout, out[-2000:]
