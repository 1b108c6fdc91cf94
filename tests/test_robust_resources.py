"""Resource budget of the firefly-robust combine (csrc/rt_robust.hip): no scratch, no spilled registers, no STATIC LDS -- the
per-lane key column and the parked ranks are dynamic LDS sized by the split at the launch; an array of keys indexed by the chunk
would show up here as scratch -- and at least four waves per SIMD by registers.  Two waves per workgroup: 64 chunks then take
40 KB, under the 64 KB a launch gets without asking.  The file is its own translation unit, so its code object is a bundle of its
own in librt_hip.so and the bundles of the other kernels do not change (tests/test_resource_table.py holds the render kernels')."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle, rtab

ROBUST = {"rt::robust_chunk_kernel"}


@pytest.fixture(scope="module")
def robust_bundle():
    return bundle("::robust_")


def test_robust_kernel_resources(robust_bundle):
    kernels = {k: v for k, v in robust_bundle.items() if "::robust_" in k}
    assert set(kernels) == ROBUST, sorted(kernels)
    assert_budget(kernels, waves=4, lds=0, workgroup=128)
    for name, d in kernels.items():
        print(name, d)


def test_the_robust_kernel_is_a_code_object_of_its_own(robust_bundle):
    """nothing but the kernel in its bundle, and it in neither the render kernels' bundle nor another pass's"""
    assert_own_code_object(robust_bundle, ROBUST, "::robust_")
    assert set(rtab.bundle_with("::noise_")) == {"rt::noise_chunk_kernel", "rt::noise_tile_kernel"}
    assert set(rtab.bundle_with("ao_kernel")) == {"void rt::ao_kernel<false>", "void rt::ao_kernel<true>"}
    assert any("combine_chunks_kernel" in k for k in rtab.extract(rtab.LIB))  # the fold the robust frame rides behind is untouched
