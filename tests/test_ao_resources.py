"""Resource budget of the ambient-occlusion kernel (csrc/rt_ao.hip).  It is held to what tests/test_aov_chain_resources.py holds the
chain kernel to -- no scratch, no spilled registers, at least four waves per SIMD by registers, the traversal stack as the only
LDS -- with more state than any other pass of its shape: a lane carries the normal, the offset origin and the random stream of its
pass in flight and two counts and the bent sum of its pixel across BOTH walks.  None of it is indexed dynamically; an array that
were would show up here as scratch.  The kernel is its own translation unit, so its code object is a bundle of its own in
librt_hip.so and the bundles of the other kernels do not change."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle, rtab

AO = {"void rt::ao_kernel<false>", "void rt::ao_kernel<true>"}


@pytest.fixture(scope="module")
def ao_bundle():
    return bundle("ao_kernel")


def test_ao_kernel_resources(ao_bundle):
    kernels = {k: v for k, v in ao_bundle.items() if "ao_kernel" in k}
    assert set(kernels) == AO, sorted(kernels)
    assert_budget(kernels, waves=4, lds=0)  # (the traversal stack is dynamic LDS, nothing else)


def test_the_ao_kernel_is_a_code_object_of_its_own(ao_bundle):
    """nothing but the AO kernel in its bundle, and none of it in the render kernels' bundle or another pass's"""
    assert_own_code_object(ao_bundle, AO, "ao_kernel")
    for word, names in (("aov_kernel", {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}),
                        ("aov_chain_kernel", {"void rt::aov_chain_kernel<false>", "void rt::aov_chain_kernel<true>"})):
        assert set(rtab.bundle_with(word)) == names, word
