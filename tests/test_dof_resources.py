"""Resource budget of the depth-of-field kernels (csrc/rt_dof.hip): no scratch, no spilled registers, and the static LDS each holds.
dof_coc_kernel holds none and runs eight waves per SIMD by registers.  dof_gather_kernel holds 52 384 bytes: the footprint of a
32 x 8 tile with a 16-pixel halo, 64 x 40 = 2560 pixels, as three colour planes of 4 bytes and one (radius, depth key) plane of 8
(51 200), the 17 x 17 table of tap distances (1 156), the four wave maxima (16), and 12 bytes of alignment between them -- below the
65 536 a launch gets without asking for more.  Occupancy: floor(163 840 / 52 384) = 3 workgroups of four waves per CU, twelve waves,
three per SIMD; the kernel's registers must allow at least those three (it needs about 40 VGPRs, which would allow eight), so the LDS
and nothing else sets the occupancy.  The file is its own translation unit, so its code object is a bundle of its own in librt_hip.so
and the bundles of the other kernels do not change (tests/test_resource_table.py holds the render kernels')."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle, rtab

GATHER_LDS = 4 * (3 * 2560) + 8 * 2560 + 4 * 17 * 17 + 16 + 12
LDS = {"rt::dof_coc_kernel": 0, "rt::dof_gather_kernel": GATHER_LDS}
DOF = set(LDS)
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def dof_bundle():
    return bundle("::dof_")


def test_dof_kernel_resources(dof_bundle):
    kernels = {k: v for k, v in dof_bundle.items() if "::dof_" in k}
    assert set(kernels) == DOF, sorted(kernels)
    for name, d in kernels.items():
        print(name, d)
    assert_budget({"rt::dof_coc_kernel": kernels["rt::dof_coc_kernel"]}, waves=8, lds=0, workgroup=256)
    assert GATHER_LDS == 52384 and GATHER_LDS <= 65536
    workgroups_per_cu = CU_LDS // GATHER_LDS
    waves_per_simd_by_lds = workgroups_per_cu * 4 // 4  # four waves per workgroup over four SIMDs
    assert (workgroups_per_cu, waves_per_simd_by_lds) == (3, 3)
    assert_budget({"rt::dof_gather_kernel": kernels["rt::dof_gather_kernel"]}, waves=waves_per_simd_by_lds, lds=GATHER_LDS, workgroup=256)


def test_the_dof_kernels_are_a_code_object_of_their_own(dof_bundle):
    """nothing but them in their bundle, and none of them in the render kernels' bundle or the bloom stage's"""
    assert_own_code_object(dof_bundle, DOF, "::dof_")
    assert not any("dof" in k for k in rtab.bundle_with("::bloom_"))
    assert any("combine_chunks_kernel" in k for k in rtab.extract(rtab.LIB))
