"""Resource budget of the ID-matte kernels (csrc/rt_matte.hip).  The layer kernel is held to what tests/test_aov_resources.py
holds the first-hit kernel to -- no scratch, no spilled registers, at least four waves per SIMD by registers -- and that is the
point of its design: the per-pixel table of eight IDs and eight counts lives in registers, reached by unrolled compare / select
code only; a dynamically indexed table would show up here as scratch.  The kernels are their own translation unit, so their code
object is a bundle of its own in librt_hip.so and the bundles of the other kernels do not change."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle, rtab

LAYER = {"void rt::matte_kernel<false>", "void rt::matte_kernel<true>"}
EXTRACT = {"void rt::matte_extract_kernel<false>", "void rt::matte_extract_kernel<true>"}


@pytest.fixture(scope="module")
def matte_bundle():
    return bundle("matte_kernel")


def test_matte_kernel_resources(matte_bundle):
    kernels = {k: v for k, v in matte_bundle.items() if "matte_kernel" in k}
    assert set(kernels) == LAYER, sorted(kernels)
    assert_budget(kernels, waves=4, lds=0)  # (the traversal stack is dynamic LDS)


def test_matte_extract_kernel_resources(matte_bundle):
    kernels = {k: v for k, v in matte_bundle.items() if "matte_extract_kernel" in k}
    assert set(kernels) == EXTRACT, sorted(kernels)
    assert_budget(kernels, waves=8)  # memory-bound: every wave the SIMD can hold
    # the staged variant keeps a selection of up to 2048 IDs in LDS, the other none
    assert kernels["void rt::matte_extract_kernel<true>"]["group_segment_fixed_size"] == 8192
    assert kernels["void rt::matte_extract_kernel<false>"]["group_segment_fixed_size"] == 0


def test_the_matte_kernels_are_a_code_object_of_their_own(matte_bundle):
    """nothing but the matte kernels in their bundle, and none of them in the render kernels' bundle or an AOV kernel's"""
    assert_own_code_object(matte_bundle, LAYER | EXTRACT, "matte")
    for word, names in (("aov_kernel", {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}),
                        ("aov_chain_kernel", {"void rt::aov_chain_kernel<false>", "void rt::aov_chain_kernel<true>"})):
        assert set(rtab.bundle_with(word)) == names, word
