"""Resource budget of the noise-estimate kernels (csrc/rt_noise.hip): no scratch, no spilled registers, full occupancy by
registers, no LDS -- the chunk kernel reads its S chunk sums twice instead of keeping them in an array (one indexed by the loop
would show up here as scratch), and the tile kernel sums across the lanes of its wave, not through LDS.  The file is its own
translation unit, so its code object is a bundle of its own in librt_hip.so and the bundles of the other kernels do not change
(tests/test_resource_table.py holds the render kernels' numbers)."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle, rtab

NOISE = {"rt::noise_chunk_kernel", "rt::noise_tile_kernel"}


@pytest.fixture(scope="module")
def noise_bundle():
    return bundle("::noise_")


def test_noise_kernel_resources(noise_bundle):
    kernels = {k: v for k, v in noise_bundle.items() if "::noise_" in k}
    assert set(kernels) == NOISE, sorted(kernels)
    assert_budget(kernels, waves=8, lds=0)  # (the shipped tile kernel is the cross-lane form)
    for name, d in kernels.items():
        print(name, d)
        assert d["waves_per_simd_by_registers"] == 8, (name, d)  # full occupancy: exactly what the SIMD holds


def test_the_noise_kernels_are_a_code_object_of_their_own(noise_bundle):
    """nothing but the two kernels in their bundle, and neither in the render kernels' bundle or another pass's"""
    assert_own_code_object(noise_bundle, NOISE, "::noise_")
    assert set(rtab.bundle_with("ao_kernel")) == {"void rt::ao_kernel<false>", "void rt::ao_kernel<true>"}
    assert any("combine_chunks_kernel" in k for k in rtab.extract(rtab.LIB))  # the fold the estimates ride behind is untouched
