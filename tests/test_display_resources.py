"""Resource budget of the display stage kernels (csrc/rt_display.hip): no scratch, no spilled registers, eight waves per SIMD by
registers for the histogram and exposure kernels and at least four for the map kernel (DESIGN.md section 12 says why it holds five).
They are their own translation unit, so their code object is an offload bundle of its own in librt_hip.so, found here as the
temporal kernels' is (tests/test_temporal_resources.py)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)
KERNELS = {"void rt::display_histogram<true>", "void rt::display_histogram<false>", "rt::display_exposure",
           "void rt::display_map<true>", "void rt::display_map<false>"}


@pytest.fixture(scope="module")
def display_bundle():
    """every kernel of the bundle that holds the display kernels"""
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()
    return rtab.bundle_with("display_")


def test_display_kernel_resources(display_bundle):
    assert set(display_bundle) == KERNELS, sorted(display_bundle)
    for name, d in display_bundle.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        need = 4 if "display_map" in name else 8
        assert d["waves_per_simd_by_registers"] >= need, (name, d)
        assert d["max_flat_workgroup_size"] == (1024 if "exposure" in name else 256), (name, d)


def test_only_display_kernels_in_the_display_bundle(display_bundle):
    assert not any(w in k for k in display_bundle for w in ("render_kernel", "aov_kernel", "denoise_", "temporal_", "quantise")), \
        sorted(display_bundle)
