"""Resource budget of the sky self-test kernel (csrc/rt_selftest.hip).  Both instantiations (tables in global memory, tables staged
in LDS) are held to no scratch, no spilled registers and eight waves per SIMD by registers (at most 64 VGPRs; built: 26 and 58) --
sky_sample and sky_pdf with one random stream and one direction live are a small part of what a render lane carries, and an array
indexed dynamically would show up as scratch.  The staged tables are dynamic LDS: no static LDS.  The device self-tests are one
translation unit, so their code object is a bundle of its own in librt_hip.so: none of them sits in the render kernels' bundle
(rt_render.hip), whose committed rows (profiles/resource_table.json, which lists the self-tests' bundle too) they cannot move."""
import pytest

from resource_budget import assert_budget, bundle, rtab

SKY = {"void rt::sky_selftest_kernel<false>", "void rt::sky_selftest_kernel<true>"}
SELFTESTS = SKY | {"rt::selftest_lean_kernel", "rt::selftest_pair_primary_kernel"}


@pytest.fixture(scope="module")
def sky_bundle():
    return bundle("sky_selftest_kernel")


def test_sky_selftest_kernel_resources(sky_bundle):
    kernels = {k: v for k, v in sky_bundle.items() if "sky_selftest_kernel" in k}
    assert set(kernels) == SKY, sorted(kernels)
    assert_budget(kernels, waves=8, lds=0)


def test_the_selftest_kernels_are_a_code_object_of_their_own(sky_bundle):
    """nothing but the self-tests in their bundle, and none of them in the render kernels' bundle"""
    assert set(sky_bundle) == SELFTESTS, sorted(sky_bundle)
    assert not any("selftest" in k for k in rtab.bundle_with("render_kernel"))
