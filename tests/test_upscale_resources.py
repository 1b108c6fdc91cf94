"""Resource budget of the upscaling kernel (csrc/rt_upscale.hip): its translation unit's bundle holds only upscale_ kernels, none
uses scratch or spills a register, the instantiations without normals (no powf) keep eight waves per SIMD by registers and those
with normals at least four (98 VGPRs: four taps' f64 powf chains interleaved; DESIGN.md section 13 says why that is kept)."""
import pytest

from resource_budget import assert_budget, bundle

B = ("false", "true")
KERNELS = {f"void rt::upscale_kernel<{a}, {n}, {z}>" for a in B for n in B for z in B}


@pytest.fixture(scope="module")
def upscale_bundle():
    return bundle("upscale_")


def test_upscale_kernel_resources(upscale_bundle):
    assert set(upscale_bundle) == KERNELS, sorted(upscale_bundle)
    for with_normals, waves in (("true", 4), ("false", 8)):
        part = {k: d for k, d in upscale_bundle.items() if k.split(", ")[1] == with_normals}
        assert_budget(part, waves=waves, lds=2 * 16 * 20 * 20)  # the 20 x 20 footprint, two float4 per source pixel


def test_only_upscale_kernels_in_the_upscale_bundle(upscale_bundle):
    assert all("upscale_" in k for k in upscale_bundle), sorted(upscale_bundle)
    assert not any(w in k for k in upscale_bundle for w in ("render_kernel", "aov_kernel", "denoise_", "temporal_", "display_", "quantise")), \
        sorted(upscale_bundle)
