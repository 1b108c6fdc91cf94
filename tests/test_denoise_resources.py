"""Resource budget of the denoiser kernels (csrc/rt_denoise.hip): no scratch, no spilled registers, at least eight waves per SIMD
by registers.  The kernels are their own translation unit, so their code object is an offload bundle of its own in librt_hip.so
(as the AOV kernel's, tests/test_aov_resources.py).  tests/probes/resource_table.py finds the bundle
(bundle_with)."""
import pytest

from resource_budget import assert_budget, bundle

KERNELS = {"void rt::denoise_prepass_kernel<0>", "void rt::denoise_prepass_kernel<1>", "void rt::denoise_prepass_kernel<2>",
           "rt::denoise_variance_kernel", "void rt::denoise_iteration_kernel<false>", "void rt::denoise_iteration_kernel<true>"}


@pytest.fixture(scope="module")
def denoise_bundle():
    """every kernel of the bundle that holds the denoiser's kernels"""
    return bundle("denoise_")


def test_denoise_kernel_resources(denoise_bundle):
    mine = {k: v for k, v in denoise_bundle.items() if "denoise_" in k}
    assert set(mine) == KERNELS, sorted(mine)
    assert_budget(mine, waves=8)


def test_no_render_or_aov_kernel_in_the_denoise_bundle(denoise_bundle):
    assert not any("render_kernel" in k or "aov_kernel" in k for k in denoise_bundle), sorted(denoise_bundle)
