"""Resource budget of the upscaling kernel (csrc/rt_upscale.hip): its translation unit's bundle holds only upscale_ kernels, none
uses scratch or spills a register, the instantiations without normals (no powf) keep eight waves per SIMD by registers and those
with normals at least four (98 VGPRs: four taps' f64 powf chains interleaved; DESIGN.md section 13 says why that is kept)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)
B = ("false", "true")
KERNELS = {f"void rt::upscale_kernel<{a}, {n}, {z}>" for a in B for n in B for z in B}


@pytest.fixture(scope="module")
def upscale_bundle():
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()
    return rtab.bundle_with("upscale_")


def test_upscale_kernel_resources(upscale_bundle):
    assert set(upscale_bundle) == KERNELS, sorted(upscale_bundle)
    for name, d in upscale_bundle.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        with_normals = name.split(", ")[1] == "true"
        assert d["waves_per_simd_by_registers"] >= (4 if with_normals else 8), (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)
        assert d["group_segment_fixed_size"] == 2 * 16 * 20 * 20, (name, d)  # the 20 x 20 footprint, two float4 per source pixel


def test_only_upscale_kernels_in_the_upscale_bundle(upscale_bundle):
    assert all("upscale_" in k for k in upscale_bundle), sorted(upscale_bundle)
    assert not any(w in k for k in upscale_bundle for w in ("render_kernel", "aov_kernel", "denoise_", "temporal_", "display_", "quantise")), \
        sorted(upscale_bundle)
