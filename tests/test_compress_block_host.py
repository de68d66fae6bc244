"""The Compress block body (vapoursynth-zip_amd/csrc/compress_block.hpp, plain C++: the text every lane of the kernel runs) on the host:
tests/compress_block_check.cpp is a stand-alone program built with the host compiler under AddressSanitizer +
UndefinedBehaviorSanitizer (without them where the compiler has no libasan) together with host_params.cpp. It runs the blocks of a
noise plane, of a natural one and of the extreme patterns through every parameter set of the GPU tests, with the luma and the chroma
tables, and the samples it writes are compared with the numpy spec's (tests/compress_ref.py), bit for bit."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import compress_ref as cr

ROOT = Path(__file__).resolve().parents[1]


def _blocks(p: np.ndarray) -> np.ndarray:
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)


@pytest.fixture(scope="module")
def blocks():
    yy, xx = np.mgrid[0:8, 0:8]
    extreme = [np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8), (((yy + xx) & 1) * 255).astype(np.uint8), ((xx & 1) * 255).astype(np.uint8),
               ((yy & 1) * 255).astype(np.uint8), ((yy >= 4) * 255).astype(np.uint8), ((xx < 4) * 255).astype(np.uint8), (yy * 36).astype(np.uint8)]
    return np.concatenate([_blocks(cr.gpu_plane(0, 64, 72)), _blocks(cr.gpu_plane(1, 64, 72)), np.stack(extreme)])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("compress_block") / "compress_block_check"
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if Path(probe).is_absolute() else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *san, str(ROOT / "tests" / "compress_block_check.cpp"),
                        str(ROOT / "vapoursynth-zip_amd" / "csrc" / "host_params.cpp"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.mark.parametrize("kw", cr.MPEG2_PARAMS + cr.JPEG_PARAMS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_block_body_equals_the_spec(exe, blocks, tmp_path, kw):
    a = dict(cr.DEFAULTS, **kw)
    tb = cr.tables(**a)
    (tmp_path / "in.bin").write_bytes(blocks.tobytes())
    for chroma in (0, 1):
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), *(str(a[k]) for k in ("codec", "qscale", "dc_prec", "quality")), str(chroma)],
                           capture_output=True, text=True, timeout=120)
        out = r.stdout + r.stderr
        assert r.returncode == 0 and f"{len(blocks)} blocks" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
        got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8).reshape(-1, 8, 8)
        level = 128 if a["codec"] == 1 else 0
        want = cr.idct(cr.quant_dequant(cr.fdct(blocks.astype(np.int32) - np.int32(level)), tb, chroma), level)
        assert np.array_equal(got, want), (kw, chroma, int((got != want).sum()))
