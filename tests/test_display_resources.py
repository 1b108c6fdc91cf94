"""Resource budget of the display stage kernels (csrc/rt_display.hip): no scratch, no spilled registers, eight waves per SIMD by
registers for the histogram and exposure kernels and at least four for the map kernel (DESIGN.md section 12 says why it holds five).
They are their own translation unit, so their code object is an offload bundle of its own in librt_hip.so, found here as the
temporal kernels' is (tests/test_temporal_resources.py)."""
import pytest

from resource_budget import assert_budget, bundle

KERNELS = {"void rt::display_histogram<true>", "void rt::display_histogram<false>", "rt::display_exposure",
           "void rt::display_map<true>", "void rt::display_map<false>"}


@pytest.fixture(scope="module")
def display_bundle():
    """every kernel of the bundle that holds the display kernels"""
    return bundle("display_")


def test_display_kernel_resources(display_bundle):
    assert set(display_bundle) == KERNELS, sorted(display_bundle)
    for part, waves, workgroup in (("display_map", 4, 256), ("display_histogram", 8, 256), ("display_exposure", 8, 1024)):
        assert_budget({k: d for k, d in display_bundle.items() if part in k}, waves=waves, workgroup=workgroup)


def test_only_display_kernels_in_the_display_bundle(display_bundle):
    assert not any(w in k for k in display_bundle for w in ("render_kernel", "aov_kernel", "denoise_", "temporal_", "quantise")), \
        sorted(display_bundle)
