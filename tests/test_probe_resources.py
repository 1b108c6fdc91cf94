"""Resources of the light-probe kernels (csrc/rt_probe.hip), the rows DESIGN.md section 25 states.  The translation unit is an
offload bundle of its own in librt_hip.so, outside the bundles profiles/resource_table.json describes, so the render kernels bench.py
measures are the parent's code object; the radiance, tiles and lens bundles hold what they held.

probe_kernel is lens_kernel (csrc/rt_lens.hip) with the direction in START and the projection in FINISH; the 27 sums of a slot live
in the caller's workspace, not in registers, so the loop carries what lens_kernel's carries.  As built: no scratch, no spilled
vector register, four waves per SIMD.  What is built is what is asserted."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle

PROBE = {f"void rt::probe_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
SMALL = {"rt::probe_zero_kernel", "rt::probe_combine_kernel", "rt::probe_eval_kernel"}
LENS = {f"void rt::lens_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
TILES = {f"void rt::tiles_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
RADIANCE = {f"void rt::radiance_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}


@pytest.fixture(scope="module")
def probe_bundle():
    return bundle("probe_kernel")


def test_the_bundle_holds_exactly_the_new_kernels(probe_bundle):
    names = set(probe_bundle)
    assert {k for k in names if "probe_kernel<" in k} == PROBE, sorted(names)
    rest = {k for k in names if "probe_kernel<" not in k}
    assert len(rest) == len(SMALL) and all(any(k.startswith(s) for k in rest) for s in SMALL), sorted(rest)
    assert_own_code_object(probe_bundle, names, "probe_")


def test_the_other_passes_keep_their_bundles():
    assert set(bundle("radiance_kernel")) == RADIANCE
    assert {k for k in bundle("tiles_kernel") if "tiles_kernel<" in k} == TILES
    lens = bundle("lens_kernel")
    assert {k for k in lens if "lens_kernel<" in k} == LENS and not any("probe" in k for k in lens)


def test_probe_kernel_budget(probe_bundle):
    """no scratch, no spilled VGPR, no static LDS (stacks and records are dynamic LDS), lens_kernel's four waves per SIMD, and not more
    vector registers than the 128 that allow them"""
    kernels = {k: v for k, v in probe_bundle.items() if "probe_kernel<" in k}
    assert_budget({k: dict(v, sgpr_spill_count=0) for k, v in kernels.items()}, waves=4, lds=0)
    for name, d in kernels.items():
        print(name, {k: d[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                       "private_segment_fixed_size", "waves_per_simd_by_registers")})
        assert d["agpr_count"] == 0 and d["vgpr_count"] <= 128
        assert d["sgpr_spill_count"] <= 64, (name, d)  # scalars parked in lanes of a VGPR: no memory behind them (scratch is 0)


def test_small_kernels_budget(probe_bundle):
    """no scratch, no spills, no LDS, full occupancy"""
    small = {k: v for k, v in probe_bundle.items() if "probe_kernel<" not in k}
    assert_budget({k: v for k, v in small.items() if "probe_zero" not in k}, waves=8, lds=0)
    for name, d in small.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["group_segment_fixed_size"] == 0 and d["waves_per_simd_by_registers"] == 8, (name, d)
