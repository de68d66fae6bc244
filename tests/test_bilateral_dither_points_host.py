"""The BilateralDither point-list generator (vapoursynth-zip_amd/csrc/host_params.cpp, plain C++) on the host:
tests/bilateral_dither_points_check.cpp is a stand-alone program built with the host compiler under AddressSanitizer +
UndefinedBehaviorSanitizer together with host_params.cpp. It sweeps radius 2 ... 48 with subspl 0, 4, 8, 16 and 4096 (every spiral
geometry, a dozen void-and-cluster ones), checks K, the leading (0, 0), uniqueness and the window per list, and prints a checksum per
geometry, which is compared with the numpy spec's (tests/bilateral_dither_ref.py)."""
import subprocess
from pathlib import Path

import pytest

import bilateral_dither_ref as bd

ROOT = Path(__file__).resolve().parents[1]
# the geometries with K >= 32 (a void-and-cluster matrix each) that the program runs: kLarge of the .cpp
LARGE = [(7, 4), (9, 8), (10, 4), (11, 4), (12, 16), (16, 4), (16, 8), (17, 0), (24, 0), (33, 16), (40, 4), (48, 4)]


def test_point_list_generator_under_asan_ubsan(tmp_path):
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not Path(probe).is_absolute():
        pytest.skip("g++ has no libasan")
    exe = tmp_path / "bilateral_dither_points_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        str(ROOT / "tests" / "bilateral_dither_points_check.cpp"), str(ROOT / "vapoursynth-zip_amd" / "csrc" / "host_params.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and ", 0 failures" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("geometry ")]
    want = [(radius, subspl) for radius in range(2, 49) for subspl in (0, 4, 8, 16, 4096) if bd.points_k(radius, subspl) < 32 or (radius, subspl) in LARGE]
    assert [(int(a), int(b)) for a, b, _, _ in rows] == want and f"{len(want)} geometries, {len(LARGE)} with K >= 32" in r.stdout, out[-2000:]
    for radius, subspl, k, total in rows:
        pts = bd.point_lists(int(radius), float(subspl))
        assert pts.shape[1] == int(k) and bd.checksum(pts) == int(total), (radius, subspl, k)
    assert sum(int(k) >= 32 for _, _, k, _ in rows) == len(LARGE) == 12
