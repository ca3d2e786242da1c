"""Register / scratch budget of the k_ec_blend kernels (kernels_blend_ec.hip), read from the code-object metadata inside
libjxl_hip.so like tests/test_blend_kernel_resources.py: a thread keeps the samples of up to four extra channels and of the
colour in registers, indexed by constants only and picked by their alpha index with selects, so none of the three
instantiations may touch scratch.

The kernel is memory-bound and should keep eight waves per SIMD (at most 64 VGPRs).  It does not: the number of extra
channels, the modes and the alpha indices are launch arguments, not template parameters, so every instantiation -- not
only the packed one -- carries the case of four channels, in which ANY channel may be the alpha of any other and of the
colour: the 32 background and foreground samples of the four planes stay live until the last plane is blended, beside
the colour's alpha terms, one channel's own terms and results, and the 64-bit addresses of up to eleven rows (forcing 64
with an occupancy attribute spills 20 to 31 registers).  Observed: 94 (save only), 96 (float RGB), 111 (packed, the
general format).  Asserted: those counts rounded up to the allocation granule of 8 -- 96, 96 and 112, all within the 128
of four waves per SIMD -- so that a change that costs an instantiation a wave shows here."""
import os

from libjxl_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CEILINGS = {"ILi0E": 96, "ILi1E": 96, "ILi2E": 112}  # OUTK: save only, linear float RGB out, packed out


def test_blend_ec_kernels_have_no_scratch():
    from libjxl_amd import build
    abi.load_library()
    so = os.path.join(ROOT, "libjxl_amd", "csrc", "libjxl_hip.so")
    res = build.kernel_resources(so)
    ks = {k: v for k, v in res.items() if "k_ec_blend" in k}
    assert len(ks) == 3, sorted(ks)
    assert not {k: v for k, v in ks.items() if v["scratch"] or v["spills"]}
    for tag, ceiling in CEILINGS.items():
        (v,) = [v for k, v in ks.items() if "k_ec_blend" + tag in k]
        print("k_ec_blend<%s>: %d VGPRs" % (tag, v["vgprs"]))
        assert v["vgprs"] <= ceiling <= 128, (tag, v["vgprs"])
    build.check_no_scratch(so, "k_ec_blend")  # what the build runs
    # k_blend is as it was: its three instantiations, and the new kernel's name is no match for its pattern
    kb = {k: v for k, v in res.items() if "k_blend" in k}
    assert len(kb) == 3 and not set(kb) & set(ks), sorted(kb)
    assert max(v["vgprs"] for v in kb.values()) <= 64
