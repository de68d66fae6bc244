"""Static check of the generated gfx950 code of depth.hip (no GPU): the error diffusion is specified with every product and every sum rounded on
its own, and hipcc contracts by default, so the kernels must hold no fused multiply-add (v_fma*, v_mac*, v_fmac*); the lane above's error
travels by a wave_shr:1 DPP move and the seam's by v_readlane."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BUILD = ROOT / "vapoursynth-zip_amd" / "csrc" / "_build"
LLVM = Path("/opt/rocm/lib/llvm/bin")


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("no ROCm LLVM tools")
    if not (BUILD / "depth.o").is_file():
        sys.path.insert(0, str(ROOT))
        import __graft_entry__ as g

        g.build()
    tmp = tmp_path_factory.mktemp("depth_isa")
    fat, dev = tmp / "fat.bin", tmp / "dev.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(BUILD / "depth.o")], check=True, capture_output=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={dev}", "--unbundle"],
                   check=True, capture_output=True)
    return subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(dev)], check=True, capture_output=True, text=True).stdout


def kernels(dis):
    """name -> instruction text of each kernel"""
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(line.strip())
    return {k: "\n".join(v) for k, v in out.items()}


def test_no_fused_multiply_add_in_any_depth_kernel(disassembly):
    ks = kernels(disassembly)
    diffuse = [k for k in ks if "depth_diffuse_kernel" in k]
    none = [k for k in ks if "depth_none_kernel" in k]
    assert len(diffuse) == 8 and len(none) == 4, sorted(ks)  # four sample-type pairs, two workgroup sizes
    for k in diffuse + none:
        fused = re.findall(r"\bv_(?:pk_)?(?:fma|mac|fmac|mad)\w*_f(?:16|32|64)\b.*", ks[k])
        assert not fused, (k, fused[:3])
        assert "v_rndne_f32" in ks[k], k  # rint, half to even


def test_errors_travel_by_dpp_and_readlane(disassembly):
    for k, text in kernels(disassembly).items():
        if "depth_diffuse_kernel" in k:
            assert "wave_shr:1" in text and "v_readlane_b32" in text and "s_barrier" in text, k
            assert "flat_load" not in text and "flat_store" not in text, k  # the carry row is an LDS or a global access, never a pointer chosen between the two
