"""Register / scratch budget of the k_blend kernels (kernels_blend.hip), read from the code-object metadata inside
libjxl_hip.so like tests/test_patches_kernel_resources.py: a thread keeps twelve background and twelve frame samples in
registers, indexed by constants only, so none of the three instantiations may touch scratch; and the kernel is
memory-bound, so it must leave the SIMDs their full eight waves."""
import os

from libjxl_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blend_kernels_have_no_scratch():
    from libjxl_amd import build
    abi.load_library()
    so = os.path.join(ROOT, "libjxl_amd", "csrc", "libjxl_hip.so")
    ks = {k: v for k, v in build.kernel_resources(so).items() if "k_blend" in k}
    assert len(ks) == 3, sorted(ks)  # save only, linear float RGB out, packed out
    assert not {k: v for k, v in ks.items() if v["scratch"] or v["spills"]}
    # observed: 32 (save only), 36 (float RGB), 54 (packed, the general format); 64 = eight waves per SIMD
    assert max(v["vgprs"] for v in ks.values()) <= 64
    build.check_no_scratch(so, "k_blend")  # what the build runs
