"""Resource budget of the bloom kernels (csrc/rt_bloom.hip): no scratch, no spilled registers, and the static LDS each holds --
bloom_reduce 21 168 bytes (the 66 x 18 x 3 footprint and the 32 x 18 x 3 horizontal pass; <true> 4 more for the exposure scale),
bloom_tail 49 152 (the 4096 pixels of its levels), bloom_composite the 4 bytes of the scale, bloom_expand_add none.  By registers
the four 256-thread kernels run eight waves per SIMD; bloom_tail's one 1024-thread workgroup is four waves per SIMD by itself and
holds the 128 registers that allows.  The file is its own translation unit, so its code object is a bundle of its own in
librt_hip.so and the bundles of the other kernels do not change (tests/test_resource_table.py holds the render kernels')."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle, rtab

LDS = {"void rt::bloom_reduce<true>": 21172, "void rt::bloom_reduce<false>": 21168, "rt::bloom_tail": 49152, "rt::bloom_expand_add": 0,
       "rt::bloom_composite": 4}
BLOOM = set(LDS)


@pytest.fixture(scope="module")
def bloom_bundle():
    return bundle("::bloom_")


def test_bloom_kernel_resources(bloom_bundle):
    kernels = {k: v for k, v in bloom_bundle.items() if "::bloom_" in k}
    assert set(kernels) == BLOOM, sorted(kernels)
    for name, d in kernels.items():
        print(name, d)
        if name == "rt::bloom_tail":
            assert_budget({name: d}, waves=4, lds=LDS[name], workgroup=1024)
        else:
            assert_budget({name: d}, waves=8, lds=LDS[name], workgroup=256)


def test_the_bloom_kernels_are_a_code_object_of_their_own(bloom_bundle):
    """nothing but them in their bundle, and none of them in the render kernels' bundle or the display stage's"""
    assert_own_code_object(bloom_bundle, BLOOM, "::bloom_")
    assert not any("bloom" in k for k in rtab.bundle_with("::display_"))
    assert any("combine_chunks_kernel" in k for k in rtab.extract(rtab.LIB))
