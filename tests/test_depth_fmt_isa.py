"""Static check of the generated gfx950 code of depth_fmt.hip (no GPU). The error diffusion from float and half sources is depth.hip's kernel,
specified with every product and every sum rounded on its own: its instantiations here hold no fused multiply-add, hand the lane above's error
down by a wave_shr:1 DPP move and the seam's by v_readlane, and make no flat access. The `none` kernels between integers and floats are specified
with ONE fused multiply-add a sample (a separate multiply and add would differ in the last bit): each holds one. Loads of the streaming kernels
keep their non-temporal hint, and no kernel spills."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BUILD = ROOT / "vapoursynth-zip_amd" / "csrc" / "_build"
LLVM = Path("/opt/rocm/lib/llvm/bin")


@pytest.fixture(scope="module")
def device_object(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("no ROCm LLVM tools")
    if not (BUILD / "depth_fmt.o").is_file():
        sys.path.insert(0, str(ROOT))
        import __graft_entry__ as g

        g.build()
    tmp = tmp_path_factory.mktemp("depth_fmt_isa")
    fat, dev = tmp / "fat.bin", tmp / "dev.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(BUILD / "depth_fmt.o")], check=True, capture_output=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={dev}", "--unbundle"],
                   check=True, capture_output=True)
    return dev


@pytest.fixture(scope="module")
def kernels(device_object):
    """demangled name -> instruction text of each kernel"""
    dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", "--demangle", str(device_object)], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(line.strip())
    return {k: "\n".join(v) for k, v in out.items() if "_kernel<" in k}


def types_of(name):
    a, b = re.search(r"_kernel<([^,>]+), ([^,>]+)", name).groups()
    return a.strip(), b.strip()


INTS, FLOATS = {"unsigned char", "unsigned short"}, {"float", "_Float16"}


def test_the_object_holds_the_kernels_of_the_entry_point_and_no_others(kernels):
    diffuse = sorted(k for k in kernels if "depth_diffuse_kernel<" in k)
    none = sorted(k for k in kernels if "depth_fmt_none_kernel<" in k)
    assert len(diffuse) == 8 and len(none) == 12 and len(kernels) == 20, sorted(kernels)
    assert {types_of(k) for k in diffuse} == {(a, b) for a in FLOATS for b in INTS}  # float sources only: the integer ones are depth.o's
    assert {types_of(k) for k in none} == {(a, b) for a in INTS | FLOATS for b in INTS | FLOATS} - {(a, b) for a in INTS for b in INTS}
    assert not any("depth_none_kernel<" in k for k in kernels)


def test_float_source_diffusion_holds_no_fused_multiply_add(kernels):
    for k, text in kernels.items():
        if "depth_diffuse_kernel<" not in k:
            continue
        fused = re.findall(r"\bv_(?:pk_)?(?:fma|mac|fmac|mad)\w*_f(?:16|32|64)\b.*", text)
        assert not fused, (k, fused[:3])
        assert "v_rndne_f32" in text, k
        assert "wave_shr:1" in text and "v_readlane_b32" in text and "s_barrier" in text, k
        assert "flat_load" not in text and "flat_store" not in text, k
        if types_of(k)[0] == "_Float16":
            assert "v_cvt_f32_f16" in text, k  # widened by the hardware's conversion at pop


def test_every_integer_float_none_kernel_fuses_its_multiply_add(kernels):
    for k, text in kernels.items():
        if "depth_fmt_none_kernel<" not in k:
            continue
        a, b = types_of(k)
        # (v_fma_mix_f32: the fused multiply-add in f32 on a half operand widened in the instruction, which is exact)
        fused = re.findall(r"\bv_(?:fma_f32|fmac_f32|pk_fma_f32|fma_mix_f32)\b", text)
        if (a in INTS) != (b in INTS):
            assert fused, k
            assert not re.search(r"\bv_(?:pk_)?mul_f32\b", text), k  # and no product rounded on its own
        else:
            assert not fused, k
        if a in FLOATS and b in INTS:
            assert "v_rndne_f32" in text, k
        assert "v_cvt_pkrtz" not in text, k  # halves are rounded to nearest even, never towards zero
        assert not re.search(r"\bv_fma_mix(?:lo|hi)_f16\b", text), k  # int -> half rounds the f32 result; a fused fma-to-half rounds once and differs
        loads = re.findall(r"\bglobal_load_dwordx[24]\b.*", text)
        assert loads and all(" nt" in l for l in loads), (k, loads[:2])
        assert "flat_load" not in text and "flat_store" not in text, k


def test_no_kernel_spills(device_object):
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(device_object)], check=True, capture_output=True, text=True).stdout
    sizes = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)]
    vgprs = [int(x) for x in re.findall(r"\.vgpr_count:\s*(\d+)", notes)]
    assert len(sizes) == 20 and not any(sizes), sizes
    assert len(vgprs) == 20 and max(vgprs) <= 64, vgprs  # the 16-wave workgroup: 1024 threads, at most 128 registers a lane; 64 keeps two workgroups a CU
