"""Resource budget of the sky self-test kernel (csrc/rt_sky_selftest.hip).  profiles/resource_table.json lists the render kernels'
bundle only, so this file stands in for a row there: both instantiations (tables in global memory, tables staged in LDS) are held
to no scratch, no spilled registers and eight waves per SIMD by registers (at most 64 VGPRs; built: 26 and 58) -- sky_sample and sky_pdf with one random stream
and one direction live are a small part of what a render lane carries, and an array indexed dynamically would show up as scratch.
The staged tables are dynamic LDS: no static LDS.  The kernel is its own translation unit, so its code object is a bundle of its own
in librt_hip.so: the render kernels' bundle, and with it every committed row of the table, does not change."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle

SKY = {"void rt::sky_selftest_kernel<false>", "void rt::sky_selftest_kernel<true>"}


@pytest.fixture(scope="module")
def sky_bundle():
    return bundle("sky_selftest_kernel")


def test_sky_selftest_kernel_resources(sky_bundle):
    kernels = {k: v for k, v in sky_bundle.items() if "sky_selftest_kernel" in k}
    assert set(kernels) == SKY, sorted(kernels)
    assert_budget(kernels, waves=8, lds=0)


def test_the_sky_selftest_kernel_is_a_code_object_of_its_own(sky_bundle):
    assert_own_code_object(sky_bundle, SKY, "sky_selftest_kernel")
