"""The arithmetic and the argument checks of vszip_depth_fmt on the host: tests/depth_fmt_check.cpp is a stand-alone program built with the host
compiler under AddressSanitizer + UndefinedBehaviorSanitizer together with csrc/host_params.cpp, and run directly; nothing is loaded into Python.
It runs the functions of csrc/depth_fmt.hpp that the kernels call over every code value of 8, 9, 10, 12 and 16 bits and over a quarter-step grid
of floats beyond both ends of the range, {limited, full} x {luma, chroma}, and prints a checksum per case, compared here with the numpy
specification (tests/depth_fmt_ref.py); and it sweeps vszip_depth_fmt_check over every refusal, whose codes and texts are compared with the
specification's check_args."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import depth_fmt_ref as df
import depth_ref as dr

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "vapoursynth-zip_amd" / "csrc"


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not Path(probe).is_absolute():
        pytest.skip("g++ has no libasan")
    exe = tmp_path_factory.mktemp("depth_fmt") / "depth_fmt_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + str(CSRC),
                        str(ROOT / "tests" / "depth_fmt_check.cpp"), str(CSRC / "host_params.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and r.stdout.rstrip().endswith("done"), out[-4000:]
    return r.stdout


def checksum(a) -> int:
    v = np.ascontiguousarray(a).reshape(-1)
    v = v.view(np.uint32) if v.dtype == np.float32 else v.astype(np.uint32)
    with np.errstate(over="ignore"):
        return int((v.astype(np.uint64) * (np.arange(v.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))


def test_the_kernels_arithmetic_is_the_specifications(check_output):
    seen = 0
    for line in check_output.splitlines():
        if not line.startswith("arith "):
            continue
        t = line.split()
        bits, full, chroma = int(t[1]), bool(int(t[2])), bool(int(t[3]))
        got = dict(zip(t[4::2], t[5::2]))
        off, rng = df.range_of(bits, full, chroma)
        assert (int(got["off"]), int(got["rng"])) == (off, rng), line
        assert int(got["mul"], 16) == int(np.float32(1.0 / rng).view(np.uint32)) and int(got["add"], 16) & 0x7FFFFFFF == int(np.float32(float(off) / rng).view(np.uint32)), line
        v = np.arange(1 << bits).astype(dr.dtype_of(bits)).reshape(1, -1)
        f = df.int_to_float(v, bits, full, chroma)
        assert int(got["to_float"]) == checksum(f), line
        assert int(got["round_trip"]) == checksum(df.float_to_int(f, bits, full, chroma)) == checksum(v), line
        k = np.arange(((1 << bits) + 16) * 4, dtype=np.float64)
        x = np.concatenate([((k * 0.25 - 8.0 - off) / rng).astype(np.float32), np.float32([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0])]).reshape(1, -1)
        assert int(got["to_int"]) == checksum(df.float_to_int(x, bits, full, chroma)), line
        seen += 1
    assert seen == 5 * 4


def test_every_refusal_has_the_specifications_code_and_text(check_output):
    served, refused = 0, {}
    for line in check_output.splitlines():
        if not line.startswith("check "):
            continue
        m = re.match(r"check (-?\d+) (-?\d+) (-?\d+) (-?\d+) (-?\d+) (-?\d+) planes (\d+)((?: -?\d+)*) -> (-?\d+) (-?\d+) (-?\d+) (\d) \|(.*)\|$", line)
        assert m, line
        args = [int(g) for g in m.groups()[:6]]
        p = [int(x) for x in m.group(8).split()]
        planes = [(bool(p[i]), bool(p[i + 1]), p[i + 2], p[i + 3], p[i + 4], p[i + 5], bool(p[i + 6])) for i in range(0, len(p), 7)]
        assert len(planes) == int(m.group(7))
        rc, quiet, cut, prefix, text = int(m.group(9)), int(m.group(10)), int(m.group(11)), int(m.group(12)), m.group(13)
        assert rc == quiet == cut and prefix == 1, line  # the same code with no buffer and with one of 8 bytes, whose text is a prefix
        try:
            df.check_args(*args, planes)
            want = (0, "")
        except dr.DepthError as e:
            want = (e.code, str(e))
        assert (rc, text) == want, (line, want)
        if rc == 0:
            served += 1
        else:
            refused[re.sub(r"-?\d+", "#", text)] = rc
    assert served >= 30
    kinds = {"DepthFmt: dtype_in # is none of VSZIP_U#, VSZIP_U#, VSZIP_F#, VSZIP_F#": -1, "DepthFmt: dtype_out # is none of VSZIP_U#, VSZIP_U#, VSZIP_F#, VSZIP_F#": -1,
             "DepthFmt: bits_in # does not fit VSZIP_U# (#..#)": -1, "DepthFmt: bits_out # does not fit VSZIP_U# (#..#)": -1, "DepthFmt: bits_in # does not fit VSZIP_U# (#)": -1,
             "DepthFmt: bits_out # does not fit VSZIP_F# (#)": -1, "DepthFmt: dither # is neither # (none) nor # (error diffusion)": -1,
             "DepthFmt: error diffusion needs an integer destination, dtype_out is VSZIP_F#": -1, "DepthFmt: no planes": -1, "DepthFmt: plane #: src and dst must not be NULL": -1,
             "DepthFmt: plane #: bad geometry #x#, pitches # -> #": -1, "DepthFmt: plane #: error diffusion from float with an offset (limited range) is not built (DESIGN.md section #)": -3,
             "DepthFmt: plane #: error diffusion from float with an offset (chroma) is not built (DESIGN.md section #)": -3, "DepthFmt: # rows are more than one call numbers": -3,
             "Depth: plane #: full-range chroma is not built (DESIGN.md section #)": -3, "Depth: no planes": -1, "Depth: dither # is neither # (none) nor # (error diffusion)": -1}
    for k, code in kinds.items():
        assert refused.get(k) == code, (k, sorted(refused))
