"""Resource budget of the ambient-occlusion kernel (csrc/rt_ao.hip).  It is held to what tests/test_aov_chain_resources.py holds the
chain kernel to -- no scratch, no spilled registers, at least four waves per SIMD by registers, the traversal stack as the only
LDS -- with more state than any other pass of its shape: a lane carries the normal, the offset origin and the random stream of its
pass in flight and two counts and the bent sum of its pixel across BOTH walks.  None of it is indexed dynamically; an array that
were would show up here as scratch.  The kernel is its own translation unit, so its code object is a bundle of its own in
librt_hip.so and the bundles of the other kernels do not change."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)

AO = {"void rt::ao_kernel<false>", "void rt::ao_kernel<true>"}


@pytest.fixture(scope="module")
def ao_bundle():
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()
    return rtab.bundle_with("ao_kernel")


def test_ao_kernel_resources(ao_bundle):
    kernels = {k: v for k, v in ao_bundle.items() if "ao_kernel" in k}
    assert set(kernels) == AO, sorted(kernels)
    for name, d in kernels.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= 4, (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)
        assert d["group_segment_fixed_size"] == 0, (name, d)  # (the traversal stack is dynamic LDS, nothing else)


def test_the_ao_kernel_is_a_code_object_of_its_own(ao_bundle):
    """nothing but the AO kernel in its bundle, and none of it in the render kernels' bundle or another pass's"""
    assert set(ao_bundle) == AO, sorted(ao_bundle)
    assert not any("ao_kernel" in k for k in rtab.extract(rtab.LIB))
    for word, names in (("aov_kernel", {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}),
                        ("aov_chain_kernel", {"void rt::aov_chain_kernel<false>", "void rt::aov_chain_kernel<true>"})):
        assert set(rtab.bundle_with(word)) == names, word
