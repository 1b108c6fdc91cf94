"""Resources of the tile-list render and the tile selection (csrc/rt_adaptive.hip).  The translation unit is an offload bundle of
its own in librt_hip.so, outside the bundles profiles/resource_table.json describes, so the render kernels bench.py measures are
the parent's code object; the radiance bundle still holds exactly its four kernels (tests/test_radiance_resources.py asserts
their rows, unchanged).

tiles_kernel is radiance_kernel's integrator (csrc/rt_path_lane.h, one copy for both: DESIGN.md section 22 has the rows before and
after the move) with a camera ray in front and the render's fold behind.  What a pixel's fold
carries between passes (sums, pass counters, the ray counter: eleven words a lane) waits in LDS behind the stacks, not in
registers: kept in registers the MIS kernels spilled 14 to 19 VGPRs.  As built: no scratch, no spilled vector register, four
waves per SIMD -- radiance_kernel's occupancy.  What is built is what is asserted."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle

TILES = {f"void rt::tiles_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
SMALL = {"rt::tiles_zero_kernel", "rt::tiles_combine_kernel", "rt::select_tiles_kernel", "rt::adaptive_fold_kernel", "rt::adaptive_fill_kernel"}
RADIANCE = {f"void rt::radiance_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}


def _named(kernels, word):
    return {k: v for k, v in kernels.items() if word in k}


@pytest.fixture(scope="module")
def adaptive_bundle():
    return bundle("tiles_kernel")


def test_the_bundle_holds_exactly_the_new_kernels(adaptive_bundle):
    names = set(adaptive_bundle)
    assert {k for k in names if "tiles_kernel<" in k} == TILES, sorted(names)
    rest = {k for k in names if "tiles_kernel<" not in k}
    assert len(rest) == len(SMALL) and all(any(k.startswith(s) for k in rest) for s in SMALL), sorted(rest)
    assert_own_code_object(adaptive_bundle, names, "tiles_")
    assert_own_code_object(adaptive_bundle, names, "adaptive_")


def test_the_other_passes_keep_their_bundles():
    assert set(bundle("radiance_kernel")) == RADIANCE
    assert set(bundle("ao_kernel")) == {"void rt::ao_kernel<false>", "void rt::ao_kernel<true>"}
    noise = bundle("::noise_")
    assert not any("tiles" in k for k in noise) and len(noise) == 2, sorted(noise)


def test_tiles_kernel_budget(adaptive_bundle):
    """no scratch, no spilled VGPR, no static LDS (stacks and fold records are dynamic LDS), waves per SIMD not below
    radiance_kernel's four"""
    kernels = _named(adaptive_bundle, "tiles_kernel<")
    assert_budget({k: dict(v, sgpr_spill_count=0) for k, v in kernels.items()}, waves=4, lds=0)
    for name, d in kernels.items():
        print(name, {k: d[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                       "private_segment_fixed_size", "waves_per_simd_by_registers")})
        assert d["agpr_count"] == 0 and d["vgpr_count"] <= 128
        assert d["sgpr_spill_count"] <= 64, (name, d)  # scalars parked in lanes of a VGPR: no memory behind them (scratch is 0)


def test_small_kernels_budget(adaptive_bundle):
    """no scratch, no spills, full occupancy; no LDS beyond the four wave counts the selection declares (the fold reads its S sums
    twice instead of keeping them in an array, which would show up here as scratch)"""
    small = {k: v for k, v in adaptive_bundle.items() if "tiles_kernel<" not in k}
    assert_budget({k: v for k, v in small.items() if "tiles_zero" not in k}, waves=8)
    for name, d in small.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["group_segment_fixed_size"] == (16 if "select_tiles" in name else 0), (name, d)
