"""Resource budget of the ID-matte kernels (csrc/rt_matte.hip).  The layer kernel is held to what tests/test_aov_resources.py
holds the first-hit kernel to -- no scratch, no spilled registers, at least four waves per SIMD by registers -- and that is the
point of its design: the per-pixel table of eight IDs and eight counts lives in registers, reached by unrolled compare / select
code only; a dynamically indexed table would show up here as scratch.  The kernels are their own translation unit, so their code
object is a bundle of its own in librt_hip.so and the bundles of the other kernels do not change."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)

LAYER = {"void rt::matte_kernel<false>", "void rt::matte_kernel<true>"}
EXTRACT = {"void rt::matte_extract_kernel<false>", "void rt::matte_extract_kernel<true>"}


@pytest.fixture(scope="module")
def matte_bundle():
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()
    return rtab.bundle_with("matte_kernel")


def test_matte_kernel_resources(matte_bundle):
    kernels = {k: v for k, v in matte_bundle.items() if "matte_kernel" in k}
    assert set(kernels) == LAYER, sorted(kernels)
    for name, d in kernels.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= 4, (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)
        assert d["group_segment_fixed_size"] == 0, (name, d)  # (the traversal stack is dynamic LDS)


def test_matte_extract_kernel_resources(matte_bundle):
    kernels = {k: v for k, v in matte_bundle.items() if "matte_extract_kernel" in k}
    assert set(kernels) == EXTRACT, sorted(kernels)
    for name, d in kernels.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= 8, (name, d)  # memory-bound: every wave the SIMD can hold
        assert d["max_flat_workgroup_size"] == 256, (name, d)
    # the staged variant keeps a selection of up to 2048 IDs in LDS, the other none
    assert kernels["void rt::matte_extract_kernel<true>"]["group_segment_fixed_size"] == 8192
    assert kernels["void rt::matte_extract_kernel<false>"]["group_segment_fixed_size"] == 0


def test_the_matte_kernels_are_a_code_object_of_their_own(matte_bundle):
    """nothing but the matte kernels in their bundle, and none of them in the render kernels' bundle or an AOV kernel's"""
    assert set(matte_bundle) == LAYER | EXTRACT, sorted(matte_bundle)
    assert not any("matte" in k for k in rtab.extract(rtab.LIB))
    for word, names in (("aov_kernel", {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}),
                        ("aov_chain_kernel", {"void rt::aov_chain_kernel<false>", "void rt::aov_chain_kernel<true>"})):
        assert set(rtab.bundle_with(word)) == names, word
