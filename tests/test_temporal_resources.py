"""Resource budget of the temporal accumulation kernels (csrc/rt_temporal.hip): no scratch, no spilled registers, a 256-thread
maximum workgroup and at least four waves per SIMD by registers (the kernels fit eight today: DESIGN.md section 11).  They are their
own translation unit, so their code object is an offload bundle of its own in librt_hip.so, found here as the denoiser's is
(tests/test_denoise_resources.py).  The denoiser's kernels are launched from it but never instantiated in it."""
import pytest

from resource_budget import assert_budget, bundle

KERNELS = {"rt::temporal_reproject", "rt::temporal_resolve", "rt::temporal_feedback"}


@pytest.fixture(scope="module")
def temporal_bundle():
    """every kernel of the bundle that holds the temporal kernels"""
    return bundle("temporal_")


def test_temporal_kernel_resources(temporal_bundle):
    assert set(temporal_bundle) == KERNELS, sorted(temporal_bundle)
    assert_budget(temporal_bundle, waves=4)


def test_no_render_aov_or_denoiser_kernel_in_the_temporal_bundle(temporal_bundle):
    assert not any(w in k for k in temporal_bundle for w in ("render_kernel", "aov_kernel", "denoise_")), sorted(temporal_bundle)
