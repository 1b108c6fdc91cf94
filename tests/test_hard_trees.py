"""The hard-tree table (tests/hard_tree_cases.py) on the CPU: the trees have the structure that makes them hard, every checker
runs on every case, twice to the same bytes, and every reference says something -- a case whose reference is all sky, all open or
all one ID would test nothing on the GPU.  Where the geometry of a case rules a condition out, the table names the reason and the
exact property that holds instead is asserted here."""
import numpy as np
import pytest

import ao_checker as A
import aov_chain_checker as KC
import aov_checker as K
import hard_tree_cases as HT
import matte_checker as M
import scenes

abi = scenes.abi
NO_ID = np.uint32(0xFFFFFFFF)
N = HT.W * HT.H


def _host(hb, sc):
    return hb.HipScene(sc, device=abi.RT_DEVICE_NONE)


def _same_bytes(a, b):
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


# ---- structure, through the host-only build ----
def test_the_chain_needs_more_than_64_kb_of_lds_and_at_most_96(hb):
    """four waves x depth x 256 B; the build refuses more than 96 entries, so 98 304 B is the most there can be"""
    sc = scenes.skewed_chain_of_spheres(HT.CHAIN_SPHERES, HT.CHAIN_RATIO, specular_every=HT.CHAIN_SPECULAR_EVERY)
    for scene in (sc, scenes.skewed_chain_of_spheres(HT.CHAIN_SPHERES, HT.CHAIN_RATIO)):
        nodes, _, depth, _ = _host(hb, scene).wide_tree()
        assert len(nodes) > 0
        assert 65536 < depth * 1024 <= 98304, depth


def test_the_default_chain_scene_is_byte_for_byte_the_old_one():
    import ctypes as C
    for n, ratio, split in ((64, 1.35, abi.RT_SPLIT_MIDDLE), (112, 1.44, abi.RT_SPLIT_MIDDLE), (7, 1.2, abi.RT_SPLIT_SAH)):
        sc = scenes.SceneDescription(split)  # the loop as it stood before the generator took `specular_every`
        mats = [sc.lambertian(sc.solid((0.8, 0.3, 0.3)), 0.8), sc.lambertian(sc.solid((0.3, 0.8, 0.3)), 0.8), sc.emissive(sc.solid((1.0, 0.9, 0.8)), 3.0)]
        x = 1.0
        for i in range(n):
            sc.sphere((x, 0.0, 0.0), 0.2 * x, mats[2] if i % 9 == 4 else mats[i % 2])
            x *= ratio
        sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (16, 8))
        new = scenes.skewed_chain_of_spheres(n, ratio, split)
        a, b = sc.desc(), new.desc()
        assert (a.n_primitives, a.n_materials, a.n_textures, a.split_type) == (b.n_primitives, b.n_materials, b.n_textures, b.split_type)
        for what, count in (("primitives", a.n_primitives), ("materials", a.n_materials)):
            pa, pb = getattr(a, what), getattr(b, what)
            size = C.sizeof(pa._type_) * count
            assert C.string_at(pa, size) == C.string_at(pb, size), what
        assert bytes(a.sky) == bytes(b.sky)
        for ta, tb in zip(sc.textures, new.textures):
            assert (ta.type, ta.colour_one[:], ta.colour_two[:]) == (tb.type, tb.colour_one[:], tb.colour_two[:])
        specular = scenes.skewed_chain_of_spheres(n, ratio, split, specular_every=3)
        kinds = [specular.materials[i].type for i in range(len(specular.materials))]
        assert abi.RT_MAT_REFLECT in kinds and abi.RT_MAT_REFRACT in kinds


def test_small_far_trees_have_a_wide_node_with_an_absent_child(hb):
    for what, sc, _ in scenes.small_far_scenes():
        nodes, _ = _host(hb, sc).wide_tree_compact()
        assert any(int(n["child"][1]) >> 26 != 0xF for n in nodes), what


def test_single_sphere_is_a_root_leaf(hb):
    assert _host(hb, scenes.single_sphere()).counts() == (1, 1, 0)


def test_every_lattice_leaf_of_one_face_is_flat(hb):
    """a leaf of two triangles is one face of a box: zero extent on one axis.  (2 of the 945 leaves hold four triangles, two faces
    of different orientation whose centroids coincide, and are not flat.)"""
    nodes = _host(hb, scenes.flat_box_lattice(np.random.default_rng(21))).nodes()
    leaves = nodes[nodes["children"][:, 0] < 0]
    flat = ((leaves["max"] - leaves["min"])[:, :3] == 0).any(axis=1)
    assert len(leaves) > 900 and flat[leaves["number_primitives"] == 2].all() and (leaves["number_primitives"] == 2).sum() > 900
    assert (~flat).sum() * 100 < len(leaves)


def test_the_tiny_trees_are_the_parity_tests_sizes():
    tiny = {name: case for name, case in HT.CASES.items() if case.primitives}
    assert len(tiny) == 14
    for name, case in tiny.items():
        assert HT.built(name)[2].counts()[1] == case.primitives, name


# ---- every checker on every case: runs, repeats its bytes, and says something ----
@pytest.mark.parametrize("name", list(HT.CASES))
def test_first_hit_reference(name):
    sc, _, cpu, cam = HT.built(name)
    r = HT.aov(name)
    assert _same_bytes(r, K.aovs(sc, cpu, cam, HT.W, HT.H, HT.SPP, seed=HT.SEED))
    hit = int((r["coverage"] > 0).sum())
    print(f"{name}: {hit} of {N} pixels hit")
    assert hit >= 10
    if HT.CASES[name].one_id:
        assert (r["coverage"] == 1.0).all(), HT.CASES[name].one_id
    else:
        assert 0 < hit < N


@pytest.mark.parametrize("name", list(HT.CASES))
def test_chain_reference(name):
    sc, _, cpu, cam = HT.built(name)
    r = HT.aov_chain(name)
    assert _same_bytes(r, KC.aovs(sc, cpu, cam, HT.W, HT.H, HT.SPP, seed=HT.SEED))
    followed = int((r["bounces"] > 0).sum())
    print(f"{name}: {followed} pixels whose terminal vertex is not the first hit, mean surfaces followed {r['bounces'].mean():.3f}")
    if HT.CASES[name].specular:
        assert followed >= 10 and r["bounces"].mean() > 0
    else:  # nothing to follow: the first-hit result, bit for bit
        first = HT.aov(name)
        assert all(r[k].tobytes() == first[k].tobytes() for k in first)
        assert (r["bounces"] == 0).all() and not np.signbit(r["bounces"]).any()


@pytest.mark.parametrize("name", list(HT.CASES))
def test_matte_reference(name):
    case = HT.CASES[name]
    ref = HT.matte(name)
    passes = HT.matte_pass_ids(name)
    for kind in HT.MATTE_KINDS:
        again = M.layers_from_pass_ids(passes[kind], HT.MATTE_LAYERS)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ref[kind], again))
    ids, coverage, residual = ref["primitive"]
    distinct = np.unique(ids[(coverage > 0) & (ids != NO_ID)])
    two_layers = int((coverage[1] > 0).sum())
    print(f"{name}: {len(distinct)} primitive IDs, {two_layers} pixels with two or more layers")
    if case.one_id:
        assert len(distinct) == 1 and two_layers == 0 and (coverage[0] == 1.0).all(), case.one_id
        return
    assert two_layers >= 5
    if case.one_primitive:
        assert len(distinct) == 1 and HT.built(name)[2].counts()[1] == 1, case.one_primitive
    else:
        assert len(distinct) >= 2
    # an extraction of one hit ID and the sky, as the GPU test asks for it
    selection = [int(distinct[0]), int(NO_ID)]
    matte = M.extract(ids, coverage, selection)
    assert matte.max() > 0 and (matte.tobytes() == M.extract(ids, coverage, selection).tobytes())


@pytest.mark.parametrize("name", list(HT.CASES))
def test_ao_reference(name):
    case = HT.CASES[name]
    _, _, cpu, cam = HT.built(name)
    free = HT.ao(name, 0.0)
    assert _same_bytes(free, A.ao(cpu, cam, HT.W, HT.H, HT.SPP, HT.RAYS, radius=0.0, seed=HT.SEED))
    rays = int(free["rays"].sum())
    occluded = rays - int(free["unoccluded"].sum())
    print(f"{name}: {occluded} of {rays} AO rays occluded without a limit")
    assert rays > 0
    if case.never_occluded:
        assert case.radius == 0.0 and occluded == 0, case.never_occluded
        assert (free["hits"] > 0).sum() >= 10 and (free["visibility"][free["hits"] > 0] == 1.0).all()
        return
    if case.enclosed:
        assert occluded == rays and (free["visibility"] == 0.0).all(), case.enclosed
    else:
        assert 0 < occluded < rays
        if case.crowded:
            assert 0.05 <= HT.occluded_share(free) <= 0.95
    limited = HT.ao(name, case.radius)
    assert _same_bytes(limited, A.ao(cpu, cam, HT.W, HT.H, HT.SPP, HT.RAYS, radius=case.radius, seed=HT.SEED))
    still = int(limited["rays"].sum()) - int(limited["unoccluded"].sum())
    opened = int((limited["open"] & ~free["open"]).sum())
    print(f"{name}: radius {case.radius}: {opened} rays change from occluded to open, {still} stay occluded")
    assert opened > 0 and 0 < still < rays and not (free["open"] & ~limited["open"]).any()


# ---- the non-finite scene in detail ----
def test_non_finite_geometry_reaches_every_checker_as_nan():
    name = "non_finite_geometry"
    first = HT.aov(name)
    hit = first["coverage"] > 0
    nan_pixel = np.isnan(first["normal"]).any(axis=1) | np.isnan(first["depth"])
    assert (nan_pixel & hit).any() and (~nan_pixel & hit).any()
    hits = HT.first_hits(name)
    nan_normal = [np.isnan(h["normal"]).any(axis=1) & (h["index"] != np.uint64(abi.NO_INDEX)) for h in hits]
    assert any(m.any() for m in nan_normal)  # AO: lambertian_sample and offset_ray are fed NaN there
    ao = HT.ao(name, 0.0)
    seen = nan_normal[0] | nan_normal[1]
    assert np.isnan(ao["bent_normal"][seen]).any()  # and the checker carries it: such a ray reaches nothing, its NaN direction is summed
    assert (ao["open"][nan_normal[0], 0, :]).all()
    assert (ao["hits"] == 0).any()  # and the frame has sky
    passes = HT.matte_pass_ids(name)["primitive"]
    assert (passes[0] != passes[1]).any()
