"""The render-variant table (tests/render_variant_cases.py) on the CPU: no entry is vacuous.  Every reference repeats its bytes,
every frame has hit pixels (and sky, where the camera is not enclosed), MIS is not NAIVE, sample_split 2 is not sample_split 1,
the shard is a proper part of the frame, the forced stack caps lie below what the walks of the chain's camera rays reach, the
small far trees still send rays across a node with an absent child, and the variant list and its expected launches cover every
value they name.  An exemption is named in the table with its reason, at most one per case, and its replacement is asserted."""
import numpy as np
import pytest

import hard_tree_cases as HT
import render_variant_cases as RV
import scenes
import wide_walk as WW

abi = scenes.abi
N = RV.W * RV.H


def test_the_cases_are_the_hard_trees_and_two_more():
    assert RV.CASES[:len(HT.CASES)] == list(HT.CASES) and set(RV.CASES[len(HT.CASES):]) == {"chain_along_axis", "all_materials"}
    assert (RV.W, RV.H, RV.SEED, RV.SPP) == (40, 27, 5, 4) and RV.H % 8
    assert RV.facts("all_materials").min_feature_set == 2  # the control that needs the full set
    assert RV.built("chain_along_axis")[0] is RV.built("chain")[0]  # one scene, two cameras


def test_at_most_one_exemption_per_case():
    named = list(RV.SPLIT_EXEMPT) + list(RV.CAP_EXEMPT)
    assert len(named) == len(set(named)) and set(named) <= set(RV.CASES)
    assert all(isinstance(reason, str) and reason for reason in [r for _, r in RV.SPLIT_EXEMPT.values()] + list(RV.CAP_EXEMPT.values()))
    assert all(set(methods) <= set(RV.METHODS) and methods for methods, _ in RV.SPLIT_EXEMPT.values())
    assert RV.SPLIT_EXEMPT["inside_glass"][0] == (abi.RT_METHOD_MIS,)  # NAIVE does tell the splits apart there


def _spare_mantissa_bits(a):
    """the fewest trailing zero bits among the 24-bit significands of the non-zero values (24: every value is zero)"""
    w = a.view(np.uint32).ravel()
    w = w[(w & 0x7FFFFFFF) != 0]
    m = ((w & 0x7FFFFF) | 0x800000).astype(np.int64)
    return int(np.log2(m & -m).min()) if len(m) else 24


@pytest.mark.parametrize("name", RV.CASES)
def test_reference(name):
    _, _, cpu, cam = RV.built(name)
    frames = {}
    for method in RV.METHODS:
        for split in (1, 2):
            img, rays = RV.oracle_frame(name, method, split)
            o = RV.options(method, "split1")
            o.sample_split = split
            again, rays_again = cpu.render(cam, o)
            assert img.dtype == np.float32 and img.shape == (RV.H, RV.W, 3)
            assert again.tobytes() == img.tobytes() and rays_again == rays and rays > 0, (method, split)
            assert not img.flags.writeable
            frames[method, split] = img
        # the chunks of sample_split 2 trace the same paths: the same rays, other roundings
        assert RV.oracle_frame(name, method, 1)[1] == RV.oracle_frame(name, method, 2)[1]
        differ = int((frames[method, 1].view(np.uint32) != frames[method, 2].view(np.uint32)).any(axis=2).sum())
        print(f"{name} m={method}: split 2 differs from split 1 on {differ} of {N} pixels")
        if method in RV.SPLIT_EXEMPT.get(name, ((), ""))[0]:
            # every value of both frames is a short dyadic number (or +0): neither fold has rounded anything
            assert differ == 0 and _spare_mantissa_bits(frames[method, 1]) >= 12, RV.SPLIT_EXEMPT[name][1]
            assert not np.signbit(frames[method, 1]).any()
        else:
            assert differ > 0
    # hit and sky pixels, by the pixel-centre rays
    miss = RV.camera_misses(name)
    hit = int((~miss).sum())
    print(f"{name}: {hit} of {N} pixel centres hit")
    assert hit >= 5  # (three_tiny_spheres: nine pixel centres of a 0.001 degree view)
    case = HT.CASES.get("chain" if name == "chain_along_axis" else name)
    if case is not None and (case.one_id or case.enclosed) and name != "chain_along_axis":
        assert hit == N, case.one_id or case.enclosed
    else:
        assert 0 < hit < N
    # MIS is another estimator wherever it has something to sample
    f = RV.facts(name)
    sky = RV.host_scene(name).sky_info()
    if f.lights or (sky["res_x"] | sky["res_y"]):
        a, b = frames[abi.RT_METHOD_NAIVE, 1], frames[abi.RT_METHOD_MIS, 1]
        assert (a.view(np.uint32) != b.view(np.uint32)).any(), "MIS == NAIVE"
        assert RV.oracle_frame(name, abi.RT_METHOD_MIS, 1)[1] != RV.oracle_frame(name, abi.RT_METHOD_NAIVE, 1)[1]


def test_the_shard_is_a_proper_part_of_the_frame():
    order = RV.shard_pixels()
    owned = order[order != RV.NO_INDEX].astype(np.int64)
    assert 0 < len(owned) < N and len(np.unique(owned)) == len(owned) and owned.max() < N
    assert len(order) > len(owned)  # ragged tiles: the packed layout carries padding entries, which stay zero
    ref, rays = RV.reference("single_sphere", abi.RT_METHOD_MIS, "shard1of3")
    frame = RV.oracle_frame("single_sphere", abi.RT_METHOD_MIS, 2)[0].reshape(-1, 3)
    assert rays is None and ref.shape == (len(order), 3) and (ref[order == RV.NO_INDEX] == 0).all()
    assert ref[order != RV.NO_INDEX].tobytes() == frame[owned].tobytes()
    for name in ("single_sphere", "spheres3_sah", "chain_along_axis"):  # the shard's own ray count: part of the frame's
        for method in RV.METHODS:
            assert 0 <= RV.oracle_shard_rays(name, method) < RV.oracle_frame(name, method, 2)[1]
        assert RV.oracle_shard_rays(name, abi.RT_METHOD_NAIVE) >= len(owned) * RV.SPP
    for shape in ("split1", "split2"):
        assert RV.reference("single_sphere", abi.RT_METHOD_MIS, shape)[0] is RV.oracle_frame("single_sphere", abi.RT_METHOD_MIS, int(shape[-1]))[0]


# ---- the structure the expected launches rest on ----
def test_which_cases_have_a_wide_tree():
    for name in RV.CASES:
        assert RV.facts(name).wide == (name not in RV.NO_WIDE_TREE), name
    assert RV.host_scene("single_sphere").counts() == (1, 1, 0)  # the root is a leaf
    nodes = RV.host_scene("non_finite_geometry").nodes()
    assert not np.isfinite(np.concatenate([nodes["min"], nodes["max"]])).all()  # non-finite bounds
    for name, reason in RV.NO_WIDE_TREE.items():  # ... and a forced fine schedule stays coarse there, whatever else is asked
        for v in RV.VARIANTS:
            for method in RV.METHODS:
                assert RV.expected_launch(name, v, method).fine == 0, (name, reason, v)


def test_no_case_is_a_pair_tree():
    """feature set 3 (one node over two single-sphere Lambertian leaves) is never expected: the premise"""
    zero = [name for name in RV.CASES if RV.facts(name).min_feature_set == 0]
    assert sorted(zero) == ["single_sphere", "three_tiny_spheres"]
    assert [RV.facts(name).n_primitives for name in sorted(zero)] == [1, 3]
    for name in RV.CASES:
        if RV.facts(name).n_primitives == 2:
            assert RV.facts(name).min_feature_set >= 1, name


def test_feature_sets_follow_the_headers_rule():
    want = {"single_sphere": 0, "three_tiny_spheres": 0, "degenerate_geometry": 2, "inside_glass": 2, "chain": 2, "chain_along_axis": 2,
            "all_materials": 2}
    for name in RV.CASES:
        assert RV.facts(name).min_feature_set == want.get(name, 1), name
        run, refused = RV.variants_for(name)
        low = RV.facts(name).min_feature_set
        assert refused == list(range(low)) and {v.feature_set for v in run} == {None} | set(range(low, 3))
        named = [i for i, v in enumerate(run) if v.feature_set is not None]
        assert named == list(range(named[0], len(run)))  # a named set cannot be taken back: those variants come last
        assert len(run) + sum(1 for v in RV.VARIANTS if v.feature_set in refused) == len(RV.VARIANTS)  # nothing dropped silently


def test_the_variant_list_covers_every_value_it_names():
    assert len(set(RV.VARIANTS)) == len(RV.VARIANTS) and RV.VARIANTS[0] == RV.AUTOMATIC
    for field, values in RV.VALUES.items():
        assert {getattr(v, field) for v in RV.VARIANTS} == set(values), field
    assert set(RV.KEYS) == set(RV.Variant._fields)
    need = [RV.Variant(0, 0, 0, 1, 0, None, 0), RV.Variant(0, 0, 0, 0, 0, None, 0), RV.Variant(1, 0, 0, 1, 0, None, 0),
            RV.Variant(1, 0, 0, 0, 0, None, 0), RV.Variant(0, 0, 0, 1, 1, None, 0)]
    need += [RV.Variant(1, 1, walk, 1, x, None, 0) for walk in (0, 1) for x in (0, 1)]
    need += [RV.Variant(1, 1, 0, 1, 0, None, cap) for cap in RV.STACK_CAPS]
    assert all(v in RV.VARIANTS for v in need)
    # the expected launches: both values of every field, over the table and on the chain that carries the caps alone
    for names in (RV.CASES, ["chain_along_axis"]):
        seen = {RV.expected_launch(name, v, m) for name in names for v in RV.variants_for(name)[0] for m in RV.METHODS}
        for field in ("fine", "pruned", "exchange") + (("scene_in_lds",) if len(names) > 1 else ()):
            assert {int(getattr(launch, field)) for launch in seen} == {0, 1}, (names, field)
    assert {launch.feature_set for launch in seen} == {2}
    # a setting the library ignores stays in the table with the launch it turns into
    mis, naive = abi.RT_METHOD_MIS, abi.RT_METHOD_NAIVE
    assert RV.expected_launch("spheres3_sah", RV.Variant(1, 0, 0, 1, 1, None, 0), mis).exchange is False  # coarse pruned
    assert RV.expected_launch("spheres3_sah", RV.Variant(0, 0, 0, 1, 1, None, 0), naive).exchange is False  # NAIVE
    assert RV.expected_launch("spheres3_sah", RV.Variant(0, 0, 0, 1, 1, None, 0), mis).exchange is True
    assert RV.expected_launch("spheres3_sah", RV.Variant(0, 1, 0, 1, 0, None, 0), mis) == RV.Launch(1, 1, 0, 1, False)
    assert RV.expected_launch("chain", RV.AUTOMATIC, mis) == RV.Launch(0, 1, 0, 2, False)  # 112 primitives: pruned
    assert RV.expected_launch("spheres5_sah", RV.AUTOMATIC, mis) == RV.Launch(0, 0, 1, 1, False)


# ---- the forced caps ----
def test_the_caps_lie_below_what_the_chains_walks_reach():
    """wide_walk.pending_entries: the pruned walk is the unpruned one until it holds a hit"""
    axis = RV.pending("chain_along_axis")
    print("chain_along_axis:", axis)
    assert axis["reached"] == RV.CHAIN_AXIS_MAX_PENDING and axis["unpruned"] >= axis["reached"]
    assert axis["depth"] == 85 and axis["reached"] < axis["depth"]  # (pending entries + the one in hand: within the worst case)
    assert RV.STACK_CAPS == (1, RV.CHAIN_AXIS_MAX_PENDING // 2, RV.CHAIN_AXIS_MAX_PENDING - 1) == (1, 42, 83)
    assert all(0 < cap < axis["reached"] for cap in RV.STACK_CAPS) and RV.MIDDLE_CAP == 42
    # the two-child tree (RT_TUNE_WALK 1, coarse launches of the chain): the same rays stay below its worst case, and above the caps
    # that the two-child variants of the table carry
    two = WW.two_child_pending(RV.host_scene("chain_along_axis"), RV.built("chain_along_axis")[3], RV.W, RV.H, stride=7)
    assert two == RV.CHAIN_AXIS_TWO_CHILD_PENDING == 56 < RV.narrow_stack_depth("chain") == 57
    assert all(v.stack_cap < two for v in RV.VARIANTS if v.walk == 1)
    # the exemption: from the side, no walk has anything to overflow
    side = RV.pending("chain")
    print("chain:", side)
    assert "chain" in RV.CAP_EXEMPT and side["reached"] == side["unpruned"] == RV.CHAIN_CAMERA_MAX_PENDING == 1
    assert not any(cap < side["reached"] for cap in RV.STACK_CAPS)


@pytest.mark.parametrize("name", ["three_tiny_spheres", "far_clump_of_triangles"])
def test_small_far_trees_send_rays_across_a_node_with_an_absent_child(name):
    p = RV.pending(name)
    print(name, p)
    assert p["rays"] > 0 and p["absent"] > 0  # (pending_entries asserts that none of them is entered)
