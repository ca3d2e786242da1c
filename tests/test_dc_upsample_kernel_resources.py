"""Register / scratch budget of k_dc_upsample8 (kernels_dc_upsample.hip), read from the code-object metadata inside
libjxl_hip.so like tests/test_tone_map_kernel_resources.py: a lane keeps its 4 x 25 weights and the 25 samples of a
neighbourhood in registers and indexes them with constants only, so the kernel may not touch scratch; and it must
leave a SIMD three waves (the shape DESIGN section 3 describes and tools/partial_bench.py measured)."""
import os

from libjxl_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dc_upsample_kernel_has_no_scratch():
    from libjxl_amd import build
    abi.load_library()
    so = os.path.join(ROOT, "libjxl_amd", "csrc", "libjxl_hip.so")
    ks = {k: v for k, v in build.kernel_resources(so).items() if "k_dc_upsample8" in k}
    assert len(ks) == 1, sorted(ks)
    assert not {k: v for k, v in ks.items() if v["scratch"] or v["spills"]}
    # observed in the build that was measured: 148 (100 of them the weights); 168 = three waves per SIMD
    assert max(v["vgprs"] for v in ks.values()) <= 168
    build.check_no_scratch(so, "k_dc_upsample8")  # what the build runs
