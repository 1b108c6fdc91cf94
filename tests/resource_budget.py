"""What the test_*_resources.py files share: tests/probes/resource_table.py loaded once as `rtab`, the bundle a kernel name lives
in, the budget every post-processing kernel is held to and the check that a pass's kernels are a code object of their own.  The
kernel names, the waves, the LDS sizes and the reasons for them stay with each file."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)


def require_built():
    """for a module-scoped fixture: skip without llvm-readelf, rebuild a library older than its sources"""
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    rtab.rebuild_if_stale()


def bundle(word):
    """every kernel of the offload bundle of the built library that holds a kernel whose name contains `word`"""
    require_built()
    return rtab.bundle_with(word)


def assert_budget(kernels, *, waves, lds=None, workgroup=256):
    """no scratch, no spilled registers, at least `waves` waves per SIMD by registers, a `workgroup`-thread maximum workgroup and,
    when `lds` is given, exactly that much static LDS"""
    assert kernels, "no kernel to hold to the budget"
    for name, d in kernels.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= waves, (name, d)
        assert d["max_flat_workgroup_size"] == workgroup, (name, d)
        if lds is not None:
            assert d["group_segment_fixed_size"] == lds, (name, d)


def assert_own_code_object(bundle, names, word):
    """nothing but `names` in the bundle, and no kernel named like `word` in the bundles the committed table describes (the render
    kernels', the batch queries', the self-tests')"""
    assert set(bundle) == names, sorted(bundle)
    assert not any(word in k for k in rtab.extract(rtab.LIB))
