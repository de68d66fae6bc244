"""Static check of the generated gfx950 code (no GPU): the streaming kernels' 16-byte accesses carry the cache hints the
source asks for. Limiter and LimitFilter read every sample once and write every sample once: all their 16-byte loads and
stores are non-temporal (`nt`), in every instantiation; AdaptiveBinarize loads plainly and stores non-temporally. The
values a kernel computes do not depend on the hint, so no other test sees it go: an optimiser pass that splits a vector
load and lets the backend merge the pieces again drops it silently (build.py FILE_FLAGS, limit_filter)."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BUILD = ROOT / "vapoursynth-zip_amd" / "csrc" / "_build"
LLVM = Path("/opt/rocm/lib/llvm/bin")
# object -> (kernel name, instantiations, input streams, loads are nt)
KERNELS = {"limiter": ("limiter_kernel", 5, 1, True), "limit_filter": ("limit_filter_kernel", 4, 3, True),
           "adaptive_binarize": ("adaptive_binarize_kernel", 1, 2, False)}


@pytest.fixture(scope="module")
def built():
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("no ROCm LLVM tools")
    if not all((BUILD / f"{o}.o").is_file() for o in KERNELS):
        sys.path.insert(0, str(ROOT))
        import __graft_entry__ as g

        g.build()
    return BUILD


def _kernels(built, obj, tmp_path):
    """symbol -> its instructions, from the gfx950 code object inside <obj>.o"""
    fat, dev = tmp_path / "fat.bin", tmp_path / "dev.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(built / f"{obj}.o")], check=True, capture_output=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={dev}", "--unbundle"],
                   check=True, capture_output=True)
    dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(dev)], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(line.strip())
    return out


@pytest.mark.parametrize("obj", list(KERNELS))
def test_16_byte_accesses_carry_their_hints(built, obj, tmp_path):
    name, count, inputs, loads_nt = KERNELS[obj]
    kernels = {s: ins for s, ins in _kernels(built, obj, tmp_path).items() if name in s}
    assert len(kernels) == count, sorted(kernels)
    for sym, ins in kernels.items():
        loads = [i for i in ins if i.startswith("global_load_dwordx4")]
        stores = [i for i in ins if i.startswith("global_store_dwordx4")]
        assert len(loads) >= inputs and len(stores) >= 1, (sym, loads, stores)  # (a kernel may hold its row loop unrolled)
        for i in stores:
            assert re.search(r"\bnt\b", i), (sym, i)
        for i in loads:
            assert bool(re.search(r"\bnt\b", i)) == loads_nt, (sym, i)
