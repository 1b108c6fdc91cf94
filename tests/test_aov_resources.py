"""Resource budget of the AOV kernel (csrc/rt_aov.hip): no scratch, no spilled registers, at least four waves per SIMD by
registers.  The kernel is its own translation unit, so its code object is an offload bundle of its own in librt_hip.so, outside the
bundles profiles/resource_table.json describes (the render kernels', the batch queries', the self-tests': rtab.extract).
tests/probes/resource_table.py finds the bundle (bundle_with)."""
import pytest

from resource_budget import assert_budget, bundle, rtab


@pytest.fixture(scope="module")
def aov_kernels():
    return {k: v for k, v in bundle("aov_kernel").items() if "aov_kernel" in k}


def test_aov_kernel_resources(aov_kernels):
    assert set(aov_kernels) == {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}, sorted(aov_kernels)
    assert_budget(aov_kernels, waves=4)


def test_render_kernels_are_not_in_the_aov_bundle(aov_kernels):
    """the committed table still describes every render kernel (the AOV pass added none to the bundles it covers)"""
    guarded = rtab.extract(rtab.LIB)
    assert not any("aov_kernel" in k for k in guarded)
    assert any("render_kernel" in k for k in guarded)
