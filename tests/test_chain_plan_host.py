"""The plan behind vszip_chain_ops (vapoursynth-zip_amd/csrc/chain_plan.hpp, plain C++) on the host: tests/chain_plan_check.cpp is a stand-alone program
built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer. It sweeps chains of 1 - 6 ops of all eleven kinds over tables of 1 - 3
plane slots and 1 - 5 frames in shuffled order with random process masks and sample sizes 1 / 2 / 4 (only the last writer of an entry writes the caller's
dst, no op reads what it or a concurrent entry writes - the temporal ops' neighbours included -, halves inside the reserved size and disjoint between
entries, unwritten entries are copies, neighbour entries equal the clamped frame arithmetic) and every malformed chain include/vszip_hip.h lists
(a gap in the frames, a (slot, frame) pair twice, mixed sizes in a slot, no frame numbers with a temporal op, a sample type a kind does not take, a slot
outside 0..2, ...). The same program prints the size and field offsets of every struct of vszip_chain_ops as the C compiler lays them out; they are
compared with the ctypes classes of vszip_amd.capi here."""
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
    exe = tmp_path_factory.mktemp("chain_plan") / "chain_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + str(ROOT / "vapoursynth-zip_amd" / "csrc"), str(ROOT / "tests" / "chain_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    return r.returncode, r.stdout


def test_chain_plan_under_asan_ubsan(check_output):
    rc, out = check_output
    assert rc == 0 and " 0 failures" in out, out[-4000:]
    m = re.search(r"(\d+) plans swept, (\d+) with a temporal op", out)
    assert m and int(m.group(1)) >= 6 * 3 * 5 * 3 * 40 and int(m.group(2)) >= 1000, out[-2000:]


def test_ctypes_structs_have_the_compilers_layout(check_output):
    """sizeof / offsetof of every vszip_chain_* struct as g++ sees include/vszip_hip.h against the ctypes classes Device.chain_ops fills"""
    from vszip_amd import capi

    _, out = check_output
    seen = {}
    for line in out.splitlines():
        if line.startswith("struct "):
            t = line.split()
            seen[t[1]] = (int(t[3]), {t[i]: int(t[i + 1]) for i in range(4, len(t), 2)})
    assert set(seen) == set(capi.CHAIN_STRUCTS), set(seen) ^ set(capi.CHAIN_STRUCTS)
    header = (ROOT / "include" / "vszip_hip.h").read_text()
    assert set(re.findall(r"typedef struct (vszip_chain_(?!stage)\w+)", header)) == set(seen)  # no struct of the entry point is left out
    for name, cls in capi.CHAIN_STRUCTS.items():
        size, offsets = seen[name]
        assert C.sizeof(cls) == size, (name, C.sizeof(cls), size)
        assert {f[0]: getattr(cls, f[0]).offset for f in cls._fields_} == offsets, name
    assert (capi.STAGE_CLAHE, capi.STAGE_COMB_MASK, capi.STAGE_COMB_MASK_MT, capi.STAGE_CHECKMATE, capi.STAGE_MOSQUITO_NR, capi.STAGE_DEBAND,
            capi.STAGE_BILATERAL_DITHER, capi.STAGE_COMPRESS) == tuple(int(v) for v in re.search(
                r"VSZIP_STAGE_CLAHE = (\d+), VSZIP_STAGE_COMB_MASK = (\d+), VSZIP_STAGE_COMB_MASK_MT = (\d+), VSZIP_STAGE_CHECKMATE = (\d+), VSZIP_STAGE_MOSQUITO_NR = (\d+), "
                r"VSZIP_STAGE_DEBAND = (\d+),\s+VSZIP_STAGE_BILATERAL_DITHER = (\d+), VSZIP_STAGE_COMPRESS = (\d+)", header).groups())
