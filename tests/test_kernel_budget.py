"""No GPU: the register budgets of the two float kernels, read from the built library's code-object metadata
(tools_dev/kernel_meta.py: the notes of every gfx950 code object; no instruction is looked at).

The echo canceller's near kernel runs four waves per SIMD, which 128 VGPRs still allow; the noise suppressor is held to five (16 and
32 kHz) and seven (8 kHz) waves per SIMD by its LDS, which 96 and 72 VGPRs allow.  The near kernel keeps a chosen set of lane-constant
values in registers for a whole launch or block (aec.hip: the head of aec_block) and sits at 127 of its 128; the heads of aec_block
and ns_frame say what else was tried inside these budgets.  An edit that tips a kernel over -- into scratch memory, or into the
next lower occupancy -- breaks no parity test and shows in nothing but the speed.  This is the guard."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools_dev"))
import kernel_meta  # noqa: E402

# kernel (its mangled name up to the first template argument: no demangler needed) -> the most VGPRs it may hold; every one of
# them with no scratch memory.  aec_near_kernel<MULT>, ns_kernel<256, CHN>, ns_kernel<128, CHN>
BUDGET = {"15aec_near_kernelILi": 128, "9ns_kernelILi256E": 96, "9ns_kernelILi128E": 72}
AT_LEAST = {"15aec_near_kernelILi": 2, "9ns_kernelILi256E": 2, "9ns_kernelILi128E": 2}  # 8 / 16 kHz; mono / two-channel


@pytest.fixture(scope="module")
def kernels():
    tools = ("llvm-objcopy", "llvm-readelf")
    if not all(os.path.exists(os.path.join(kernel_meta.LLVM, t)) for t in tools):
        pytest.skip("the ROCm llvm tools are not installed (%s)" % kernel_meta.LLVM)
    from wmix_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libwmix_amd.so is not built"
    return {name: dict(zip(kernel_meta.FIELDS, v)) for name, v in kernel_meta.kernels(_lib.LIB_PATH).items()}


@pytest.mark.parametrize("pattern", sorted(BUDGET))
def test_kernel_stays_inside_its_register_budget(kernels, pattern):
    mine = {n: m for n, m in kernels.items() if pattern in n}
    assert len(mine) >= AT_LEAST[pattern], "instantiations of %s found: %s" % (pattern, sorted(mine))
    for name, m in sorted(mine.items()):
        print("%s: %d VGPRs, %d AGPRs, %d B scratch" % (name[:60], m["vgpr"], m["agpr"], m["scratch"]))
        assert m["scratch"] == 0, "%s spills %d bytes per lane to scratch memory" % (name, m["scratch"])
        assert m["vgpr"] + m["agpr"] <= BUDGET[pattern], "%s holds %d registers, budget %d" % (name, m["vgpr"] + m["agpr"], BUDGET[pattern])
