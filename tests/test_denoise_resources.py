"""Resource budget of the denoiser kernels (csrc/rt_denoise.hip): no scratch, no spilled registers, at least eight waves per SIMD
by registers.  The kernels are their own translation unit, so their code object is an offload bundle of its own in librt_hip.so
(as the AOV kernel's, tests/test_aov_resources.py).  tests/probes/resource_table.py finds the bundle
(bundle_with)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)
KERNELS = {"void rt::denoise_prepass_kernel<0>", "void rt::denoise_prepass_kernel<1>", "void rt::denoise_prepass_kernel<2>",
           "rt::denoise_variance_kernel", "void rt::denoise_iteration_kernel<false>", "void rt::denoise_iteration_kernel<true>"}


@pytest.fixture(scope="module")
def denoise_bundle():
    """every kernel of the bundle that holds the denoiser's kernels"""
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()
    return rtab.bundle_with("denoise_")


def test_denoise_kernel_resources(denoise_bundle):
    mine = {k: v for k, v in denoise_bundle.items() if "denoise_" in k}
    assert set(mine) == KERNELS, sorted(mine)
    for name, d in mine.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= 8, (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)


def test_no_render_or_aov_kernel_in_the_denoise_bundle(denoise_bundle):
    assert not any("render_kernel" in k or "aov_kernel" in k for k in denoise_bundle), sorted(denoise_bundle)
