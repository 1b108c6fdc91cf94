"""The kernels' register / spill / scratch / LDS numbers are part of the product's performance (DESIGN.md section 4 records
3.5 % and 6 % losses from edits that only perturbed register allocation), so the table of the shipped library is committed as
profiles/resource_table.json and a build whose DEFAULT kernels differ from it fails here: whoever changes a kernel has to
rebuild, look at the difference (`python tests/probes/resource_table.py --diff`), measure, and commit the new table with the change."""
import json

import pytest

from resource_budget import require_built, rtab


@pytest.fixture(scope="module")
def built_table():
    require_built()  # the table must describe THESE sources
    return rtab.extract(rtab.LIB)


def test_committed_table_describes_the_current_sources():
    table = json.load(open(rtab.TABLE))
    assert table["source_hash"] == rtab.source_hash(), (
        "kernel sources changed since profiles/resource_table.json was written: rebuild (make -C raytracing-rust_amd/csrc), "
        "review `python tests/probes/resource_table.py --diff`, then `--write` and commit the table with the change")


def test_default_kernels_match_the_committed_table(built_table):
    committed = json.load(open(rtab.TABLE))["kernels"]
    default_built = {k: v for k, v in built_table.items() if v["default"]}
    default_committed = {k: v for k, v in committed.items() if v["default"]}
    assert len(default_built) >= 30 + 4  # 30 render instantiations the library selects from + the batch-query kernels
    differences = rtab.diff(default_built, default_committed)
    assert not differences, "\n".join(differences)


def test_headline_kernels_hold_their_budgets(built_table):
    """the kernels of BASELINE configs 2 and 3 and the general spheres-only kernel (coarse schedule, MIS).  Round 4 found that one
    more wave per SIMD is worth 4 - 10 % to these issue-bound kernels, more than a few dozen spilled registers cost: the register
    budgets are declared for SIX waves (spheres-only: 80 VGPRs) and FIVE (triangles + lights: 96), measured against the unconstrained
    kernels on one box (rt_render.hip RT_SPHERES_COARSE_WAVES / RT_SIMPLE_COARSE_WAVES)"""
    spheres = built_table["void rt::render_kernel<1, false, false, true, rt::Feat<false, false, false, false>, false>"]
    simple = built_table["void rt::render_kernel<1, false, false, true, rt::Feat<true, true, false, false>, false>"]
    simple_global_sky = built_table["void rt::render_kernel<1, false, false, false, rt::Feat<true, true, false, false>, false>"]  # what config 3 launches
    assert spheres["waves_per_simd_by_registers"] >= 6
    assert simple["waves_per_simd_by_registers"] >= 5 and simple_global_sky["waves_per_simd_by_registers"] >= 5
    # what those budgets cost, as measured: anything above is a regression of the code, not of the budget
    assert spheres["private_segment_fixed_size"] <= 32 and spheres["vgpr_spill_count"] <= 8
    assert spheres["sgpr_spill_count"] <= 24
    assert simple["vgpr_spill_count"] <= 44 and simple_global_sky["vgpr_spill_count"] <= 34
    assert simple["private_segment_fixed_size"] <= 100 and simple_global_sky["private_segment_fixed_size"] <= 72
    # the kernel BASELINE config 2 itself runs (rtweekend1's tree is one node over two single-sphere leaves: rt_types.h FeatPair,
    # the general walk not compiled in, material types known from what was hit, the scene itself read from the kernel
    # arguments once per super-phase): at most 80 VGPRs = six waves per SIMD WITHOUT a spilled vector register, no scratch, since the
    # persistent loop stopped keeping the lane state in two register sets (101 VGPRs before); two loop-invariant 64-bit scalars
    # may sit in lanes of a VGPR (a v_readlane pair per iteration each), nothing else.
    pair = built_table["void rt::render_kernel<1, false, false, true, rt::FeatPair, false>"]
    assert pair["waves_per_simd_by_registers"] >= 6
    assert pair["private_segment_fixed_size"] == 0 and pair["vgpr_spill_count"] == 0 and pair["sgpr_spill_count"] <= 4
