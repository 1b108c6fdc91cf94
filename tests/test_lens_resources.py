"""Resources of the lens-camera kernels (csrc/rt_lens.hip).  The translation unit is an offload bundle of its own in librt_hip.so,
outside the bundles profiles/resource_table.json describes, so the render kernels bench.py measures are the parent's code object;
the radiance, tiles, AO and noise bundles hold what they held.

lens_kernel is tiles_kernel (csrc/rt_adaptive.hip) with the camera model in START; the camera's vectors are read from the kernel
arguments where START uses them, so the loop carries what tiles_kernel's carries.  As built: no scratch, no spilled vector
register, four waves per SIMD.  What is built is what is asserted."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle

LENS = {f"void rt::lens_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
SMALL = {"rt::lens_zero_kernel", "rt::lens_combine_kernel"}
TILES = {f"void rt::tiles_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
TILES_SMALL = {"rt::tiles_zero_kernel", "rt::tiles_combine_kernel", "rt::select_tiles_kernel", "rt::adaptive_fold_kernel", "rt::adaptive_fill_kernel"}
RADIANCE = {f"void rt::radiance_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}


@pytest.fixture(scope="module")
def lens_bundle():
    return bundle("lens_kernel")


def test_the_bundle_holds_exactly_the_new_kernels(lens_bundle):
    names = set(lens_bundle)
    assert {k for k in names if "lens_kernel<" in k} == LENS, sorted(names)
    rest = {k for k in names if "lens_kernel<" not in k}
    assert len(rest) == len(SMALL) and all(any(k.startswith(s) for k in rest) for s in SMALL), sorted(rest)
    assert_own_code_object(lens_bundle, names, "lens_")


def test_the_other_passes_keep_their_bundles():
    assert set(bundle("radiance_kernel")) == RADIANCE
    tiles = set(bundle("tiles_kernel"))
    assert {k for k in tiles if "tiles_kernel<" in k} == TILES
    rest = {k for k in tiles if "tiles_kernel<" not in k}
    assert len(rest) == len(TILES_SMALL) and all(any(k.startswith(s) for k in rest) for s in TILES_SMALL), sorted(rest)
    assert set(bundle("ao_kernel")) == {"void rt::ao_kernel<false>", "void rt::ao_kernel<true>"}
    noise = bundle("::noise_")
    assert not any("lens" in k or "tiles" in k for k in noise) and len(noise) == 2, sorted(noise)


def test_lens_kernel_budget(lens_bundle):
    """no scratch, no spilled VGPR, no static LDS (stacks and fold records are dynamic LDS), at least tiles_kernel's four waves per
    SIMD, and not more vector registers than the 128 that allow them"""
    kernels = {k: v for k, v in lens_bundle.items() if "lens_kernel<" in k}
    assert_budget({k: dict(v, sgpr_spill_count=0) for k, v in kernels.items()}, waves=4, lds=0)
    for name, d in kernels.items():
        print(name, {k: d[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                       "private_segment_fixed_size", "waves_per_simd_by_registers")})
        assert d["agpr_count"] == 0 and d["vgpr_count"] <= 128
        assert d["sgpr_spill_count"] <= 64, (name, d)  # scalars parked in lanes of a VGPR: no memory behind them (scratch is 0)


def test_small_kernels_budget(lens_bundle):
    """no scratch, no spills, no LDS, full occupancy"""
    small = {k: v for k, v in lens_bundle.items() if "lens_kernel<" not in k}
    assert_budget({k: v for k, v in small.items() if "lens_zero" not in k}, waves=8, lds=0)
    for name, d in small.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["group_segment_fixed_size"] == 0 and d["waves_per_simd_by_registers"] == 8, (name, d)
