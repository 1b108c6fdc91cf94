"""The radiance table (tests/radiance_cases.py) on the CPU, oracle only: every entry is in the regime it is there for and its
reference says something, before any GPU is involved -- a sky whose MIS reference equalled its NAIVE one would never reach
sample_lights, a 64-bit stream whose reference equalled that of its low word would let a kernel drop the high word.  Every cached
reference is computed a second time and repeats its bytes.  The structure of the hard trees themselves (depths, absent children,
flat leaves) is what test_hard_trees.py asserts on the same hard_tree_cases.CASES; it is not restated here."""
import numpy as np
import pytest

import hard_tree_cases as HT
import radiance_cases as RC
import scenes
import sky_cases as SK

abi = scenes.abi
NO_INDEX = np.uint64(0xFFFFFFFFFFFFFFFF)
# Where a ray set provably cannot do what the others do, the reason, and the exact property asserted instead:
#   no_hit       no ray of the set reaches a primitive: both references are the sky's emission, equal bit for bit and non-zero
#   black_paths  every MIS sample is exactly zero although every ray hits
TREE_EXCEPTIONS = {
    "three_tiny_spheres": ("no_hit", "the first four rows of the 16 x 9 grid pass above the 7e-5 clump the 0.001-degree frame is aimed at, and "
                           "every probe starts 1e-3 outside it pointing away: the walks cross the root's node and find nothing"),
    "inside_glass": ("black_paths", "every ray starts inside the glass sphere: the first vertex is a delta material, whose eval and "
                     "scattering pdf are 0, so under MIS both the light sample and the power heuristic's material weight vanish"),
}


def _host(hb, sc):
    return hb.HipScene(sc, device=abi.RT_DEVICE_NONE)


def _hits(key):
    o, d, _ = RC.rays(key)
    rec = RC.built(key)[2].check_hit(o, d)
    return (rec["found"] != 0) & (rec["index"] != NO_INDEX)


def _differs(a, b):
    """per ray: any value differs (NaN != NaN does not count)"""
    return ((a != b) & ~(np.isnan(a) & np.isnan(b))).any(axis=tuple(range(1, a.ndim)))


def _repeats(key, method):
    ref = RC.reference(key, method)
    again = RC.compute(key, method, RC.ENTRIES[key].k)
    assert ref.dtype == again.dtype == np.float64 and ref.tobytes() == again.tobytes(), (key, method)
    return ref


# ---- the table itself ----
def test_the_table_covers_every_case_of_the_two_tables_it_is_built_from():
    assert [k.split("/")[1] for k in RC.TREES] == list(HT.CASES)
    assert "negative" not in SK.RENDER_CASES and len(SK.RENDER_CASES) == len(SK.CASES) - 1
    for case in SK.RENDER_CASES:
        scenes_of = [k.split("/")[2] for k in RC.SKIES if k.split("/")[1] == case]
        assert scenes_of == (["floor"] if case in SK.HUGE else ["floor", "spheres", "lit_spheres"]), case
    for key in RC.SKIES:
        e = RC.ENTRIES[key]
        o, d, centres = RC.rays(key)
        huge = key.split("/")[1] in SK.HUGE
        assert (len(o), centres, e.k) == ((64, 32, 1) if huge else (128, 64, 2)), key
    for key in RC.TREES:
        o, d, centres = RC.rays(key)
        assert centres == 64 and 64 <= len(o) <= 128 and RC.ENTRIES[key].k == 2, key
    o, d, centres = RC.rays("streams")
    assert len(o) == 257 and centres == 144
    st = RC.streams()
    assert st.dtype == np.uint64 and st.shape == (257,)
    assert all(int((st == np.uint64(v)).sum()) >= 8 for v in RC.STREAM_VALUES) and set(int(s) for s in st) == set(RC.STREAM_VALUES)
    assert RC.sample_indices((1 << 32) - 1) == [(1 << 32) - 1, 1 << 32, (1 << 32) + 1]  # the carry, mid-ray
    assert RC.sample_indices((1 << 64) - 2) == [(1 << 64) - 2, (1 << 64) - 1, 0]        # the wrap


# ---- hard trees ----
@pytest.mark.parametrize("key", RC.TREES)
def test_tree_reference(key):
    name = key.split("/")[1]
    naive, mis = _repeats(key, RC.NAIVE), _repeats(key, RC.MIS)
    hit = _hits(key)
    walked = int(_differs(naive[:, 0], naive[:, 1]).sum())  # the two samples differ: the path bounced and drew
    print(f"{key}: {len(hit)} rays, {int(hit.sum())} reach a primitive, NAIVE samples 0 and 1 differ on {walked}, "
          f"MIS != NAIVE on {int(_differs(naive, mis).sum())}")
    assert np.isfinite(naive).all() and np.isfinite(mis).all()  # (non_finite_geometry: the NaN filter of both integrators)
    kind, why = TREE_EXCEPTIONS.get(name, (None, None))
    if kind == "no_hit":
        assert not hit.any() and naive.tobytes() == mis.tobytes() and (naive != 0).any(axis=(1, 2)).all(), why
        return
    assert hit.any()
    assert (naive != 0).any()
    if kind == "black_paths":
        assert hit.all() and (mis == 0).all(), why
    else:
        assert (mis != 0).any()


def test_the_chain_needs_more_than_64_kb_of_dynamic_lds(hb):
    sc = RC.built("tree/chain")[0]
    nodes, _, depth, _ = _host(hb, sc).wide_tree()  # rt_scene_wide_info's stack depth
    assert len(nodes) > 0
    assert RC.four_wave_lds_bytes(depth) == 87040 > 65536, depth
    assert (160 * 1024) // RC.four_wave_lds_bytes(depth) == 1  # path_lane_groups: one workgroup a CU


# ---- sky regimes ----
@pytest.mark.parametrize("key", RC.SKIES)
def test_sky_reference(hb, key):
    _, case, scene = key.split("/")
    naive, mis = _repeats(key, RC.NAIVE), _repeats(key, RC.MIS)
    sc = RC.built(key)[0]
    if case not in SK.HUGE:  # (a host build of a 2^24-cell table: test_sky_tables.py does it once, for the same texture and resolution)
        host = _host(hb, sc)
        si = host.sky_info()
        assert (si["res_x"], si["res_y"]) == tuple(SK.CASES[case].res) and si["guide_k"] == SK.CASES[case].guide_k, key
        assert si["inv_res_ok"] == SK.CASES[case].inv_res_ok
        assert (host.counts()[2] > 0) == (scene == "lit_spheres")
    differing = int(_differs(naive, mis).sum())
    print(f"{key}: MIS != NAIVE on {differing} of {len(mis)} rays, MIS non-zero on {int((mis != 0).any(axis=(1, 2)).sum())}")
    assert np.isfinite(mis).all(), key
    if case == "black" and scene != "lit_spheres":
        # The sky is the only emitter and its texture is 0: every emission term of either integrator is exactly +0, a light
        # sample's `eval * weight * 0 / l_pdf` with l_pdf == 0 is NaN and is filtered to 0 (mis.rs:88-90).  So MIS is exactly 0
        # on every ray and cannot differ from NAIVE; what the GPU must reproduce here is the filter.
        assert (mis == 0).all() and (naive == 0).all() and _hits(key).any()
        return
    assert differing >= 1, key


# ---- the four arms of sample_lights ----
@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_sample_lights_shape(hb, name):
    key = f"shape/{name}"
    naive, mis = _repeats(key, RC.NAIVE), _repeats(key, RC.MIS)
    host = _host(hb, RC.built(key)[0])
    si = host.sky_info()
    shape = (host.counts()[2] > 0, (si["res_x"] | si["res_y"]) != 0)  # (csrc/rt_shade.h sky_can_sample)
    assert shape == RC.SHAPES[name][0], (name, shape)
    assert RC.ENTRIES[key].k == RC.SHAPE_K == 4
    hit = _hits(key)
    differs = _differs(naive, mis)
    print(f"{key}: {host.counts()[2]} emissive primitives, sampler {si['res_x']} x {si['res_y']}; {int(hit.sum())} of {len(hit)} rays reach a "
          f"primitive, MIS != NAIVE on {int(differs.sum())}")
    assert np.isfinite(mis).all() and (mis != 0).any() and differs.any()
    if name == "nothing":
        # (0, false): sample_lights returns None and every emission is added unweighted, so MIS is NAIVE's estimator -- but not
        # its bytes: the prologue scatters a CLONE of the ray (mis.rs:25), whose draws are spent and thrown away, so from the
        # first bounce on the MIS path runs two draws behind the NAIVE path of the same stream.  (The floor is Lambertian:
        # no delta material is involved.)  What does hold exactly: the two are equal on every ray that leaves without a hit
        # (no draw is used), and on this scene they differ on every ray that does hit the floor.
        assert (differs == hit).all() and hit.any() and (~hit).any()
    if name == "sky_alone":
        assert host.counts()[2] == 0
    all_shapes = {RC.SHAPES[n][0] for n in RC.SHAPES}
    assert all_shapes == {(False, True), (False, False), (True, False), (True, True)}


# ---- streams, seeds, sample indices: a dropped high word changes the reference ----
def _share(a, b, rows=None):
    d = _differs(a, b)
    return float((d if rows is None else d[rows]).mean())


@pytest.mark.parametrize("method", RC.METHODS)
def test_a_dropped_high_word_changes_at_least_a_quarter_of_the_rays(method):
    st = RC.streams()
    seed = RC.SEEDS[0]
    for value in RC.STREAM_VALUES:
        if value > RC.LOW:
            rows = st == np.uint64(value)
            share = _share(RC.stream_sample(method, seed, 0), RC.stream_sample(method, seed, 0, low_streams=True), rows)
            print(f"method {method}: stream {value:#x} against {value & RC.LOW:#x}: {share:.3f} of its {int(rows.sum())} rays differ")
            assert share >= 0.25, (value, share)
    for s in RC.SEEDS:
        if s > RC.LOW:
            share = _share(RC.stream_sample(method, s, 0), RC.stream_sample(method, s & RC.LOW, 0))
            print(f"method {method}: seed {s:#x} against its low word: {share:.3f}")
            assert share >= 0.25, (s, share)
    checked = 0
    for begin in RC.SAMPLE_BEGINS:
        for j, index in enumerate(RC.sample_indices(begin)):
            cut = ((begin & RC.LOW) + j) & RC.LOW  # a 32-bit sample_begin + k
            if cut != index:
                share = _share(RC.stream_sample(method, seed, index), RC.stream_sample(method, seed, cut))
                print(f"method {method}: sample_begin {begin:#x} + {j}: index {index:#x} against {cut:#x}: {share:.3f}")
                assert share >= 0.25, (begin, j, share)
                checked += 1
    assert checked == 2 + 3 + 2  # 2^32 - 1: k = 1, 2; 2^32: every k; 2^64 - 2: k = 0, 1 (k = 2 wraps to 0 in 64 bits as in 32)


@pytest.mark.parametrize("method", RC.METHODS)
def test_stream_references_repeat_and_are_their_single_samples_folded(method):
    """the m-sample means at (seed, stream_i, sample_begin) are the f64 means of the single samples at sample_begin + j mod 2^64:
    the carry into the high word and the wrap are the oracle's 64-bit addition"""
    for seed in RC.SEEDS:
        for begin in RC.SAMPLE_BEGINS:
            ref = RC.stream_reference(method, seed, begin)
            singles = np.stack([RC.stream_sample(method, seed, i) for i in RC.sample_indices(begin)], axis=1)
            assert np.isfinite(ref).all()
            acc = np.zeros_like(singles[:, 0])
            for j in range(RC.STREAM_K):
                acc = acc + singles[:, j]
                assert (acc / float(j + 1)).tobytes() == ref[:, j].tobytes(), (seed, begin, j)
    seed, begin = RC.SEEDS[1], RC.SAMPLE_BEGINS[1]
    again = RC.compute("streams", method, RC.STREAM_K, seed=seed, per_ray_streams=RC.streams(), sample_begin=begin)
    assert again.tobytes() == RC.stream_reference(method, seed, begin).tobytes()


# ---- the oracle's new entry against the old one ----
def test_stream_zero_from_sample_zero_is_the_old_entry_double_for_double(O):
    import ctypes as C
    cpu, cam = O.Scene(scenes.all_materials()), O.camera_new(**scenes.ALL_MATERIALS_CAMERA)
    import radiance_checker as R
    o, d = R.pixel_centre_rays(cam, 4, 2)
    assert len(o) == 8
    differing = 0
    for method in RC.METHODS:
        for i in range(8):
            for m in range(1, 5):
                ray = abi.RayDesc()
                ray.origin, ray.direction = O._f3(o[i]), O._f3(d[i])
                old = (C.c_double * 3)()
                O._check(O.lib().ora_integrate_ray(cpu._h, C.byref(ray), C.c_int32(method), C.c_uint32(50), C.c_uint32(3), C.c_uint64(5),
                                                   C.c_uint64(m), C.c_uint32(1), old))
                new = cpu.integrate_ray(o[i], d[i], method, m, seed=5, n_threads=1, stream=0, sample_begin=0)
                assert new.tobytes() == np.array(list(old)).tobytes() == cpu.integrate_ray(o[i], d[i], method, m, seed=5, n_threads=1).tobytes()
                differing += int(new.tobytes() != cpu.integrate_ray(o[i], d[i], method, m, seed=5, n_threads=1, stream=1).tobytes())
    assert differing > 0  # (and the stream argument is not ignored)


def test_sample_two_to_the_32_plus_one_is_sample_one_from_two_to_the_32(O):
    cpu, cam = O.Scene(scenes.all_materials()), O.camera_new(**scenes.ALL_MATERIALS_CAMERA)
    import radiance_checker as R
    o, d = R.pixel_centre_rays(cam, 4, 2)
    moved = 0
    for method in RC.METHODS:
        for i in range(8):
            kw = dict(seed=5, n_threads=1)
            direct = cpu.integrate_ray(o[i], d[i], method, 1, sample_begin=(1 << 32) + 1, **kw)
            first = cpu.integrate_ray(o[i], d[i], method, 1, sample_begin=1 << 32, **kw)
            both = cpu.integrate_ray(o[i], d[i], method, 2, sample_begin=1 << 32, **kw)
            assert ((first + direct) / 2.0).tobytes() == both.tobytes()  # (each a widened f32: the sum is the oracle's own add)
            moved += int(direct.tobytes() != cpu.integrate_ray(o[i], d[i], method, 1, sample_begin=1, **kw).tobytes())
            # the wrap: sample 2 from 2^64 - 2 is sample 0 (the oracle's mean: f64 adds in order from 0.0, one division)
            s0, s1, s2 = (cpu.integrate_ray(o[i], d[i], method, 1, sample_begin=b, **kw) for b in ((1 << 64) - 2, (1 << 64) - 1, 0))
            wrapped = cpu.integrate_ray(o[i], d[i], method, 3, sample_begin=(1 << 64) - 2, **kw)
            assert (((s0 + s1) + s2) / 3.0).tobytes() == wrapped.tobytes()
    assert moved > 0  # sample 2^32 + 1 is not sample 1
