"""Register / scratch budget of the k_modular_planes kernels (kernels_modular.hip), read from the code-object metadata
inside libjxl_hip.so like tests/test_modular_kernel_resources.py does for their sibling k_modular_emit: the same run of
eight pixels per lane plus, at most, one more plane -- no instantiation may touch scratch, and each must leave the SIMDs
their full eight waves.  The library must hold exactly the instantiations the launch table names: one per line of
JXLHIP_MODULAR_PLANES_KERNELS in the source."""
import os
import re

from libjxl_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_table():
    src = open(os.path.join(ROOT, "libjxl_amd", "csrc", "kernels_modular.hip")).read()
    body = src[src.index("#define JXLHIP_MODULAR_PLANES_KERNELS(X)"):]
    body = body[:body.index("\n\n")]
    return re.findall(r"^\s*X\((\w+), (\d), (\w+), (\w+), (-?\w+)\)", body, re.M)


def test_modular_planes_kernels_have_no_scratch_and_keep_eight_waves():
    from libjxl_amd import build
    abi.load_library()
    so = os.path.join(ROOT, "libjxl_amd", "csrc", "libjxl_hip.so")
    ks = {k: v for k, v in build.kernel_resources(so).items() if "k_modular_planes" in k}
    table = launch_table()
    # {int16, int32} x {grey, grey + alpha, RGB + alpha} through the general packed tail; grey to three floats; the fixed
    # 8-bit tails: RGB + alpha to RGBA8 from both sample types, 8-bit grey images to RGB8 / RGBA8 with and without alpha
    assert len(table) == len(set(table)) == 13, table
    assert len(ks) == len(table), sorted(ks)
    assert not {k: v for k, v in ks.items() if v["scratch"] or v["spills"]}
    # observed in the build that was measured: 64 / 64 (RGB + alpha, general tail, int16 / int32), 59 / 55 (RGB + alpha to
    # RGBA8), 56 and 50 (grey with and without alpha, general), 26 .. 41 (the others); 64 = eight waves per SIMD
    assert max(v["vgprs"] for v in ks.values()) <= 64, {k: v["vgprs"] for k, v in ks.items()}
    build.check_no_scratch(so, "k_modular_planes")  # what the build runs
    # RGB without alpha never comes here: it is k_modular_emit's, whose eight instantiations are untouched
    assert not [t for t in table if t[1] == "3" and t[2] == "false"]
    assert len([k for k in build.kernel_resources(so) if "k_modular_emit" in k]) == 8
