"""Resource budget of the temporal accumulation kernels (csrc/rt_temporal.hip): no scratch, no spilled registers, a 256-thread
maximum workgroup and at least four waves per SIMD by registers (the kernels fit eight today: DESIGN.md section 11).  They are their
own translation unit, so their code object is an offload bundle of its own in librt_hip.so, found here as the denoiser's is
(tests/test_denoise_resources.py).  The denoiser's kernels are launched from it but never instantiated in it."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)
KERNELS = {"rt::temporal_reproject", "rt::temporal_resolve", "rt::temporal_feedback"}


@pytest.fixture(scope="module")
def temporal_bundle():
    """every kernel of the bundle that holds the temporal kernels"""
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()
    return rtab.bundle_with("temporal_")


def test_temporal_kernel_resources(temporal_bundle):
    assert set(temporal_bundle) == KERNELS, sorted(temporal_bundle)
    for name, d in temporal_bundle.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= 4, (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)


def test_no_render_aov_or_denoiser_kernel_in_the_temporal_bundle(temporal_bundle):
    assert not any(w in k for k in temporal_bundle for w in ("render_kernel", "aov_kernel", "denoise_")), sorted(temporal_bundle)
