"""Resource budget of the specular-chain AOV kernel (csrc/rt_aov_chain.hip), held to what tests/test_aov_resources.py holds the
first-hit kernel to: no scratch, no spilled registers, at least four waves per SIMD by registers.  The kernel is its own
translation unit, so its code object is a bundle of its own in librt_hip.so and the bundles of the other kernels do not change."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)


@pytest.fixture(scope="module")
def chain_bundle():
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()
    return rtab.bundle_with("aov_chain_kernel")


def test_aov_chain_kernel_resources(chain_bundle):
    kernels = {k: v for k, v in chain_bundle.items() if "aov_chain_kernel" in k}
    assert set(kernels) == {"void rt::aov_chain_kernel<false>", "void rt::aov_chain_kernel<true>"}, sorted(kernels)
    for name, d in kernels.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= 4, (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)


def test_the_chain_kernel_is_a_code_object_of_its_own(chain_bundle):
    """nothing but the two chain kernels in its bundle, and neither in the render kernels' bundle nor the first-hit kernel's"""
    assert all("aov_chain_kernel" in k for k in chain_bundle), sorted(chain_bundle)
    assert not any("aov_chain_kernel" in k for k in rtab.extract(rtab.LIB))
    first_hit = {k for k in rtab.bundle_with("aov_kernel") if "aov" in k}
    assert first_hit == {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}, sorted(first_hit)
