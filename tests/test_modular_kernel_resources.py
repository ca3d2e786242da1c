"""Register / scratch budget of the k_modular_emit kernels (kernels_modular.hip), read from the code-object metadata inside
libjxl_hip.so like tests/test_tone_map_kernel_resources.py: a thread keeps a run of eight pixels in registers and indexes
it with constants only, so none of the eight instantiations may touch scratch; the kernel does nothing but stream, so it
must leave the SIMDs their full eight waves."""
import os

from libjxl_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_modular_emit_kernels_have_no_scratch_and_keep_eight_waves():
    from libjxl_amd import build
    abi.load_library()
    so = os.path.join(ROOT, "libjxl_amd", "csrc", "libjxl_hip.so")
    ks = {k: v for k, v in build.kernel_resources(so).items() if "k_modular_emit" in k}
    # int16 and int32 planes x (float RGB out; packed out: the general format, 8-bit RGB and RGBA fixed)
    assert len(ks) == 8, sorted(ks)
    assert not {k: v for k, v in ks.items() if v["scratch"] or v["spills"]}
    # observed in the build that was measured, int16 / int32 planes: 46 / 36 (float RGB), 64 / 64 (packed, general),
    # 54 / 59 (RGB8), 60 / 56 (RGBA8); 64 = eight waves per SIMD
    assert max(v["vgprs"] for v in ks.values()) <= 64, {k: v["vgprs"] for k, v in ks.items()}
    build.check_no_scratch(so, "k_modular_emit")  # what the build runs
