"""Register / scratch budget of the k_tone_map kernels (kernels_tonemap.hip), read from the code-object metadata inside
libjxl_hip.so like tests/test_blend_kernel_resources.py: a thread keeps two pixels in registers and indexes nothing, so
none of the four instantiations may touch scratch; the launch moves the bytes of an emit-only launch, so it must leave the SIMDs
their full eight waves."""
import os

from libjxl_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tone_map_kernels_have_no_scratch():
    from libjxl_amd import build
    abi.load_library()
    so = os.path.join(ROOT, "libjxl_amd", "csrc", "libjxl_hip.so")
    ks = {k: v for k, v in build.kernel_resources(so).items() if "k_tone_map" in k}
    assert len(ks) == 4, sorted(ks)  # linear float RGB out; packed out: the general format, 8-bit sRGB RGB and RGBA fixed
    assert not {k: v for k, v in ks.items() if v["scratch"] or v["spills"]}
    # observed in the build that was measured: 35 (float RGB), 61 (packed, general), 58 (sRGB RGB8), 48 (sRGB RGBA8);
    # 64 = eight waves per SIMD
    assert max(v["vgprs"] for v in ks.values()) <= 64
    build.check_no_scratch(so, "k_tone_map")  # what the build runs
