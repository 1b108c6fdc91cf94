"""Resources of the lens-camera AOV kernel (csrc/rt_aov_lens.hip).  The translation unit is an offload bundle of its own in
librt_hip.so, outside the bundles profiles/resource_table.json describes, so the render kernels bench.py measures are the parent's
code object; the first-hit, chain, lens, tiles and radiance bundles hold what they held.

aov_lens_guide_kernel is aov_chain_kernel (csrc/rt_aov_chain.hip) with the camera model in its `fresh` arm; the camera's vectors are
read from the kernel arguments where an arm uses them, so the loop carries what aov_chain_kernel's carries.  Its name is chosen so
that no substring look-up of the other resource files ("lens_kernel", "aov_kernel", "aov_chain_kernel", "ao_kernel") finds it.  As
built: no scratch, no spilled register, no AGPR, no static LDS (the stacks are dynamic LDS), the four waves per SIMD its launch
bounds ask for."""
import pytest

from resource_budget import assert_budget, assert_own_code_object, bundle

GUIDE = {"void rt::aov_lens_guide_kernel<false>", "void rt::aov_lens_guide_kernel<true>"}
LENS = {f"void rt::lens_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
TILES = {f"void rt::tiles_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}
RADIANCE = {f"void rt::radiance_kernel<{method}, {prune}>" for method in (0, 1) for prune in ("false", "true")}


@pytest.fixture(scope="module")
def guide_bundle():
    return bundle("aov_lens_guide_kernel")


def test_the_bundle_holds_exactly_the_new_kernels(guide_bundle):
    assert_own_code_object(guide_bundle, GUIDE, "aov_lens")


def test_the_kernel_budget(guide_bundle):
    """no scratch, no spilled register, no static LDS, four waves per SIMD: at most 128 vector registers, none of them an AGPR"""
    assert_budget(guide_bundle, waves=4, lds=0)
    for name, d in guide_bundle.items():
        print(name, {k: d[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                       "private_segment_fixed_size", "waves_per_simd_by_registers")})
        assert d["agpr_count"] == 0 and d["vgpr_count"] <= 128, (name, d)


def test_the_other_passes_keep_their_bundles():
    assert set(bundle("aov_kernel<")) == {"void rt::aov_kernel<false>", "void rt::aov_kernel<true>"}
    assert set(bundle("aov_chain_kernel")) == {"void rt::aov_chain_kernel<false>", "void rt::aov_chain_kernel<true>"}
    assert {k for k in bundle("lens_kernel") if "lens_kernel<" in k} == LENS
    assert not any("aov" in k for k in bundle("lens_kernel"))
    assert {k for k in bundle("tiles_kernel") if "tiles_kernel<" in k} == TILES
    assert set(bundle("radiance_kernel")) == RADIANCE
