"""Register conditions of the fixed-shape fused synthesis kernels: the four non-split
synth_frame_kernel instantiations that launches without a frame prefix take must leave 8 waves per SIMD (16
workgroups of two waves per CU) open, whatever residency the launch plan then ships: no scratch, at most 64
VGPRs (the allocation granule is 8; 512 / 64 = 8 waves) and SGPRs s with ceil(s / 16) * 16 + 16 <= 100.  Read
from the built library's code-object metadata (llvm-readelf, no GPU).  The any-shape forms, which lost their
pinned names to the fixed ones, keep their sine loops at the fast placement (llvm-objdump)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "ddsp_pytorch_amd", "lib", "libddsp_hip.so")

# <RNG, SPLIT = false, CTRL, PREFIX = false>
FIXED = ("synth_frame_kernelILb1ELb0ELb0ELb0EE", "synth_frame_kernelILb0ELb0ELb0ELb0EE",
         "synth_frame_kernelILb1ELb0ELb1ELb0EE", "synth_frame_kernelILb0ELb0ELb1ELb0EE")


# the any-shape forms <RNG, CTRL, PREFIX> that took over every other shape: tests/test_loop_align.py pins the
# names above, which used to be these kernels, so their sine loops' placement is held here
ANY_SHAPE = ("synth_frame_any_kernelILb1ELb0ELb0EE", "synth_frame_any_kernelILb0ELb0ELb0EE",
             "synth_frame_any_kernelILb1ELb1ELb0EE", "synth_frame_any_kernelILb0ELb1ELb0EE")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libddsp_hip.so not built (make)")
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="llvm-objdump not available")
@pytest.mark.parametrize("kernel", ANY_SHAPE)
def test_any_shape_sine_loops_at_fast_placement(kernel):
    import loop_align
    rs = loop_align.analyze_all(LIB, kernel)
    assert len(rs) == 2, f"the shared-count and the per-sample loop expected in {kernel}: {rs}"
    for r in rs:
        assert r["sines"] >= 8
        assert r["odd_dword"] >= 0.9 * r["eight_byte"], (kernel, r)


@pytest.fixture(scope="module")
def resources():
    import kres
    return kres.kernels(LIB)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libddsp_hip.so not built (make)")
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="llvm-readelf not available")
@pytest.mark.parametrize("kernel", FIXED)
def test_fixed_shape_kernel_keeps_eight_waves_per_simd_open(resources, kernel):
    rows = [r for r in resources if kernel in r[0]]
    assert len(rows) == 1, (kernel, [r[0] for r in rows])
    _, vgpr, sgpr, _, scratch = rows[0]
    print(f"{kernel}: vgpr {vgpr} sgpr {sgpr} scratch {scratch}")
    assert scratch == 0
    assert 0 < vgpr <= 64
    assert 0 < sgpr and -(-sgpr // 16) * 16 + 16 <= 100
