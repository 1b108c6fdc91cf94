"""Resources of the radiance-query kernels (csrc/rt_radiance.hip).  Their translation unit is an offload bundle of its own in
librt_hip.so, outside the bundles profiles/resource_table.json describes; the AO, AOV and chain bundles still hold exactly their
kernels.

Registers: the yardstick is the kernel these stand beside, the general fine-schedule MIS render kernel
`render_kernel<1, true, false, false, rt::Feat<true, true, true, true>, false>` of the committed table (96 VGPRs, 40 of them
spilled, 88 bytes of scratch, five waves per SIMD).  The aim -- no more VGPRs and no more spills at no fewer waves -- is MISSED on
one count: the MIS kernels need 124 VGPRs, four waves per SIMD, with nothing spilled and no scratch (DESIGN.md section 21 states
the gap with both rows).  What is built is what is asserted."""
import json

import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle, rtab

NAMES = {f"void rt::radiance_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
YARDSTICK = "void rt::render_kernel<1, true, false, false, rt::Feat<true, true, true, true>, false>"


@pytest.fixture(scope="module")
def radiance_bundle():
    return bundle("radiance_kernel")


def test_the_radiance_kernels_are_a_code_object_of_their_own(radiance_bundle):
    assert_own_code_object(radiance_bundle, NAMES, "radiance_kernel")


def test_the_other_passes_keep_their_bundles():
    assert set(bundle("ao_kernel")) == {"void rt::ao_kernel<false>", "void rt::ao_kernel<true>"}
    assert {k for k in bundle("aov_kernel<") if "aov_kernel" in k} == {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}
    assert set(bundle("aov_chain_kernel")) == {"void rt::aov_chain_kernel<false>", "void rt::aov_chain_kernel<true>"}
    for word in ("ao_kernel", "aov_kernel<", "aov_chain_kernel", "render_kernel", "check_hit"):
        assert not any("radiance_kernel" in k for k in bundle(word)), word


def test_budget(radiance_bundle):
    """no scratch at all (so none beyond spills), no spilled vector register, no static LDS (the stacks are dynamic LDS), four
    waves per SIMD"""
    assert_budget({k: dict(v, sgpr_spill_count=0) for k, v in radiance_bundle.items()}, waves=4, lds=0)
    for name, d in radiance_bundle.items():
        print(name, {k: d[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                       "private_segment_fixed_size", "waves_per_simd_by_registers")})
        assert d["agpr_count"] == 0
        assert d["sgpr_spill_count"] <= 64, (name, d)  # scalars parked in lanes of a VGPR: no memory behind them (scratch is 0)
    naive = [d for k, d in radiance_bundle.items() if "<0," in k]
    mis = [d for k, d in radiance_bundle.items() if "<1," in k]
    assert len(naive) == len(mis) == 2
    assert all(d["vgpr_count"] <= 104 for d in naive)
    assert all(d["vgpr_count"] <= 124 for d in mis)


def test_against_the_yardstick_row(radiance_bundle):
    """fewer spills and less scratch than the render kernel beside it; the VGPRs and the waves are where the aim is missed, and
    the assertion says by how much"""
    row = json.load(open(rtab.TABLE))["kernels"][YARDSTICK]
    assert (row["vgpr_count"], row["vgpr_spill_count"], row["private_segment_fixed_size"], row["waves_per_simd_by_registers"]) == (96, 40, 88, 5)
    for name, d in radiance_bundle.items():
        assert d["vgpr_spill_count"] <= row["vgpr_spill_count"] and d["private_segment_fixed_size"] <= row["private_segment_fixed_size"], name
        assert d["vgpr_count"] + d["vgpr_spill_count"] <= row["vgpr_count"] + row["vgpr_spill_count"], name  # 124 against 136
        assert d["waves_per_simd_by_registers"] == row["waves_per_simd_by_registers"] - 1, name  # the gap: four waves, not five
