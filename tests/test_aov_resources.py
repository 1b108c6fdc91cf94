"""Resource budget of the AOV kernel (csrc/rt_aov.hip): no scratch, no spilled registers, at least four waves per SIMD by
registers.  The kernel is its own translation unit, so its code object is a second offload bundle in librt_hip.so, after the
render kernels' bundle that profiles/resource_table.json describes.  tests/probes/resource_table.py finds the bundle
(bundle_with)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)


@pytest.fixture(scope="module")
def aov_kernels():
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()
    return {k: v for k, v in rtab.bundle_with("aov_kernel").items() if "aov_kernel" in k}


def test_aov_kernel_resources(aov_kernels):
    assert set(aov_kernels) == {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}, sorted(aov_kernels)
    for name, d in aov_kernels.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= 4, (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)


def test_render_kernels_are_not_in_the_aov_bundle(aov_kernels):
    """the committed table still describes every render kernel (the AOV pass added none to rt_render.hip's bundle)"""
    first = rtab.extract(rtab.LIB)
    assert not any("aov_kernel" in k for k in first)
    assert any("render_kernel" in k for k in first)
