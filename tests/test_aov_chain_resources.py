"""Resource budget of the specular-chain AOV kernel (csrc/rt_aov_chain.hip), held to what tests/test_aov_resources.py holds the
first-hit kernel to: no scratch, no spilled registers, at least four waves per SIMD by registers.  The kernel is its own
translation unit, so its code object is a bundle of its own in librt_hip.so and the bundles of the other kernels do not change."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle, rtab

CHAIN = {"void rt::aov_chain_kernel<false>", "void rt::aov_chain_kernel<true>"}


@pytest.fixture(scope="module")
def chain_bundle():
    return bundle("aov_chain_kernel")


def test_aov_chain_kernel_resources(chain_bundle):
    kernels = {k: v for k, v in chain_bundle.items() if "aov_chain_kernel" in k}
    assert set(kernels) == CHAIN, sorted(kernels)
    assert_budget(kernels, waves=4)


def test_the_chain_kernel_is_a_code_object_of_its_own(chain_bundle):
    """nothing but the two chain kernels in its bundle, and neither in the render kernels' bundle nor the first-hit kernel's"""
    assert_own_code_object(chain_bundle, CHAIN, "aov_chain_kernel")
    first_hit = {k for k in rtab.bundle_with("aov_kernel") if "aov" in k}
    assert first_hit == {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}, sorted(first_hit)
