"""The ImageUnpack lane bodies (vapoursynth-zip_amd/csrc/image_unpack_body.hpp, plain C++: the text every lane of the kernels runs) on
the host: tests/image_unpack_body_check.cpp is a stand-alone program built with the host compiler under AddressSanitizer +
UndefinedBehaviorSanitizer (without them where the compiler has no libasan). It runs the 256 lanes of every workgroup over heap blocks
of the exact size, for every required combination at widths around the unit, the wave and the workgroup's sweep, with dense source rows
(and for rgb24 rows padded to 4 bytes), on the unit path and pixel by pixel, and the planes it writes are compared with the numpy
spec's (tests/image_unpack_ref.py), bit for bit."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import image_unpack_ref as iu

ROOT = Path(__file__).resolve().parents[1]
WIDTHS = [1, 3, 4, 5, 13, 16, 17, 64, 1031, 4117]  # 4117: more than one sweep of 256 units at 16 pixels a unit, too
H = 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("image_unpack_body") / "image_unpack_body_check"
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if Path(probe).is_absolute() else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *san, str(ROOT / "tests" / "image_unpack_body_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


CASES = [(combo, None) for combo in iu.COMBOS] + [((iu.RGB, np.uint8, 8), 4)]  # (combination, source rows padded to a multiple of)


@pytest.mark.parametrize("vec", [1, 0], ids=["units", "per_pixel"])
@pytest.mark.parametrize("combo,pad", CASES, ids=[iu.combo_id(c) + ("-padded4" if p else "") for c, p in CASES])
def test_lane_bodies_equal_the_spec(exe, tmp_path, combo, pad, vec):
    layout, dt, bits = combo
    S, C = np.dtype(dt).itemsize, iu.CHANNELS[layout]
    pal = iu.palette(1) if layout == iu.INDEXED else None
    if pal is not None:
        (tmp_path / "pal.bin").write_bytes(pal.tobytes())
    for k, w in enumerate(WIDTHS):
        packed = iu.content(7 + k, H, w, combo)
        pitch = w * C * S if pad is None else -(-w * C * S // pad) * pad
        src = iu.row_bytes(packed, pitch).reshape(-1)[:(H - 1) * pitch + w * C * S]  # nothing behind the last row's pixels
        (tmp_path / "in.bin").write_bytes(src.tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "pal.bin") if pal is not None else "-", str(S), str(C), str(w), str(H),
                            str(pitch), str(vec), str(bits)], capture_output=True, text=True, timeout=120)
        out = r.stdout + r.stderr
        assert r.returncode == 0 and f"planes of {w}x{H}" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, (w, out[-4000:])
        p, a = iu.unpack(packed, layout, bits, pal)
        if layout in (iu.BGR, iu.BGRA):
            p = p[::-1]  # the program writes the planes in the pixel's memory order; exchanging R and B is the host's part
        want = p + ([a] if a is not None else [])
        got = np.frombuffer((tmp_path / "out.bin").read_bytes(), iu.bits_of(want[0]).dtype).reshape(len(want), H, w)
        for c, x in enumerate(want):
            assert np.array_equal(got[c], iu.bits_of(x)), (iu.combo_id(combo), w, vec, c, int((got[c] != iu.bits_of(x)).sum()))
