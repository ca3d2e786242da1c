"""Register / scratch budget of the k_patches kernels (kernels_patches.hip), read from the code-object metadata inside
libjxl_hip.so like tests/test_kernel_resources.py: a thread keeps its 4 x 3 samples in registers across the record
loop, so none of the four instantiations may touch scratch."""
import os

from libjxl_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_patch_kernels_have_no_scratch():
    from libjxl_amd import build
    abi.load_library()
    so = os.path.join(ROOT, "libjxl_amd", "csrc", "libjxl_hip.so")
    ks = {k: v for k, v in build.kernel_resources(so).items() if "k_patches" in k}
    assert len(ks) == 4, sorted(ks)  # blend-in-place + three output kinds
    assert not {k: v for k, v in ks.items() if v["scratch"] or v["spills"]}
    assert max(v["vgprs"] for v in ks.values()) <= 64  # eight waves per SIMD
    build.check_no_scratch(so, "k_patches")  # what the build runs
