"""vszip_color_map_lut (vapoursynth-zip_amd/csrc/host_params.cpp, plain C++) in a stand-alone program: tests/color_map_lut_check.cpp is built with the
host compiler under AddressSanitizer + UndefinedBehaviorSanitizer (without them where the compiler has no libasan) together with
host_params.cpp, with g++'s own contraction rule, not the library's -ffp-contract=off. It reads palettes of every length of
tests/color_map_ref.py from a file (each in heap blocks of exactly its size) and writes the tables, which are compared with the numpy spec's, bit
for bit; the palettes that the library refuses come back with their status and message."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import color_map_ref as cm

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("color_map_lut") / "color_map_lut_check"
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if Path(probe).is_absolute() else []
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", *san, str(ROOT / "tests" / "color_map_lut_check.cpp"),
                        str(ROOT / "vapoursynth-zip_amd" / "csrc" / "host_params.cpp"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def _palettes():
    pals = [np.stack(cm.analytic_palette(name)) for name in sorted(cm.ANALYTIC)]
    rng = np.random.default_rng(7)
    for n in cm.LENGTHS:
        pals += [rng.random((3, n), dtype=np.float32) for _ in range(20)]
    pals.append(np.stack([np.array([0.20607343316078186, 0.6694883108139038], np.float32)] * 3))  # a fused interpolation gives another byte
    bad = []
    for value in (np.float32("nan"), np.float32(1.01), np.float32(-0.01)):
        p = rng.random((3, 11), dtype=np.float32)
        p[1, 0] = value  # point 0 is table entry 0 itself
        bad.append(p)
    return pals, bad


def test_tables_equal_the_spec(exe, tmp_path):
    pals, bad = _palettes()
    with open(tmp_path / "in.bin", "wb") as f:
        for p in pals + bad:
            f.write(struct.pack("<i", p.shape[1]) + np.ascontiguousarray(p, np.float32).tobytes())
        f.write(struct.pack("<i", 0))  # len = 0
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    total = len(pals) + len(bad) + 1
    assert r.returncode == 0 and f"{total} palettes" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    rec = 4 + 768 + 128
    assert len(raw) == total * rec
    for k, p in enumerate(pals):
        rc, = struct.unpack_from("<i", raw, k * rec)
        got = np.frombuffer(raw, np.uint8, 768, k * rec + 4).reshape(3, 256)
        assert rc == 0 and np.array_equal(got, cm.lut(*p)), (k, p.shape)
    for k in range(len(pals), total):
        rc, = struct.unpack_from("<i", raw, k * rec)
        msg = raw[k * rec + 772:(k + 1) * rec].split(b"\0")[0].decode()
        assert rc == -1 and msg.startswith("ColorMap: g: table entry" if k < total - 1 else "ColorMap: len = 0"), (k, rc, msg)
