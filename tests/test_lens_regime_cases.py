"""The lens-render table (tests/lens_regime_cases.py) on the CPU, oracle and checker only: every entry is in the regime it is there
for and its reference can show the property it is there for, before any GPU is involved -- a 64-bit first sample whose frame
equalled that of its low word would let the kernel drop the high word, a fisheye of 220 degrees none of whose samples looks
backwards would never change the sign of forward * cos(theta), a lens none of whose origins lies inside the ground would be the
small lens again.  These are conditions on the inputs, not measurements of the kernel.  The oracle's counted fixed-ray integrator,
from which every ray count of the table comes, is pinned first.  Each reference test prints, per entry, whether the reference
frame holds a NaN (the only entries for which the GPU comparison may treat NaNs as equal), its inside samples and its ray count."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import lens_cases as LN
import lens_checker as LC
import lens_regime_cases as LR
import noise_checker as N
import radiance_cases as RC
import scenes
import sky_cases as SK
import tiles_cases as TC

abi = scenes.abi
F32 = np.float32
NAIVE, MIS = LR.NAIVE, LR.MIS
NO_INDEX = np.uint64(abi.NO_INDEX)


def _same(a, b, nan_equal=False):
    same = a.view(np.uint32) == b.view(np.uint32)
    if nan_equal:
        same = same | (np.isnan(a) & np.isnan(b))
    return bool(same.all())


def _differ(a, b):
    """(h, w) bool: pixels that differ in any channel (NaN against NaN does not count)"""
    return ((a != b) & ~(np.isnan(a) & np.isnan(b))).any(axis=-1)


# ---- the table itself ----
def test_the_table_has_the_groups_the_kernel_needs():
    assert len(SK.RENDER_CASES) == 14 and len(SK.HUGE) == 2
    assert len(LR.SKIES) == 12 * 6 + 2 * 4 and len(LR.ARMS) == 16 and len(LR.UNEVENS) == 12
    assert len(LR.STREAMS) == 2 * 2 * 3 * 4 and len(LR.DEPTH_KEYS) == 2 * 2 * 6 and len(LR.RAGGEDS) == 20 and len(LR.CAMERAS) == 14
    assert len(LR.ENTRIES) == sum(map(len, LR.GROUPS.values())) == 214
    for case in SK.RENDER_CASES:
        got = sorted(k.split("/", 2)[2] for k in LR.SKIES if k.split("/")[1] == case)
        floor = ["floor/mis", "floor/mis/fisheye", "floor/naive", "floor/naive/fisheye"]
        assert got == (floor if case in SK.HUGE else floor + ["lit_spheres/mis", "spheres/mis"]), case
    for key, e in LR.ENTRIES.items():
        assert e.w >= 2 and e.h >= 2 and 1 <= e.split <= e.spp and e.projection in abi.PROJECTIONS, key
        assert e.w * e.h * e.spp <= 2000 and e.w * e.h * e.spp <= 24 * 13 * 8, key  # one oracle call a sample, from Python
        assert (e.w, e.h) in ((24, 8), (8, 24)) or (e.w <= 16 and e.h <= 16), key
    assert [LR.ENTRIES[k].groups for k in LR.UNEVENS].count((0, 1)) == 2  # (7, 3), both methods
    assert [(LR.ENTRIES[k].spp, LR.ENTRIES[k].split) for k in LR.UNEVENS[:6]] == list(TC.UNEVEN)
    # ragged frames: every size under two projections at least, all four across the sizes, 2 x 2 under all four
    by_size = {}
    for k in LR.RAGGEDS:
        by_size.setdefault((LR.ENTRIES[k].w, LR.ENTRIES[k].h), set()).add(LR.ENTRIES[k].projection)
    assert set(by_size) == {(2, 2), (5, 11), (9, 8), (16, 8)} and all(len(p) >= 2 for p in by_size.values())
    assert by_size[(2, 2)] == set(abi.PROJECTIONS) == set().union(*by_size.values())
    assert not LR.padding(16, 8).any() and LR.padding(2, 2).sum() == 60 and LR.padding(5, 11).any() and LR.padding(9, 8).any()
    # the stream entries go through the thin lens: four camera draws a sample
    assert all(LR.ENTRIES[k].projection == "perspective" and LR.ENTRIES[k].aperture > 0 for k in LR.STREAMS + LR.ARMS)
    assert TC.pass_indices((1 << 32) - 2, 4) == [(1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]
    assert N.chunk_bounds(4, 2)[1] == 2  # pass 2 of 2^32 - 2 is 2^32: the first pass of the second chunk
    assert TC.pass_indices((1 << 64) - 2, 4) == [(1 << 64) - 2, (1 << 64) - 1, 0, 1]


# ---- 0. the oracle's counted fixed-ray integrator ----
def _c_ray(O, o, d):
    ray = abi.RayDesc()
    ray.origin, ray.direction = O._f3(o), O._f3(d)
    return ray


def test_the_counted_entry_is_exported_declared_and_the_old_entries_double_for_double(O):
    lib = O.lib()
    for name in ("ora_integrate_ray", "ora_integrate_ray_stream", "ora_integrate_ray_stream_counted"):
        assert hasattr(lib, name), name
    header = open(os.path.join(scenes.ROOT, "oracle", "rt_oracle.h")).read()
    assert "int ora_integrate_ray_stream_counted(" in header and "uint64_t *rays_shot);" in header
    cpu = RC.built("streams")[2]
    o, d, _ = RC.rays("streams")
    args = (C.c_uint32(50), C.c_uint32(3), C.c_uint64(5))
    for method in RC.METHODS:
        for i in range(0, 64, 7):
            ray = _c_ray(O, o[i], d[i])
            for m in (1, 3):
                old, stream, counted, quiet = ((C.c_double * 3)() for _ in range(4))
                rays = C.c_uint64(1 << 40)
                O._check(lib.ora_integrate_ray(cpu._h, C.byref(ray), C.c_int32(method), *args, C.c_uint64(m), C.c_uint32(1), old))
                O._check(lib.ora_integrate_ray_stream(cpu._h, C.byref(ray), C.c_int32(method), *args, C.c_uint64(m), C.c_uint32(1), stream,
                                                      C.c_uint64(0), C.c_uint64(0)))
                O._check(lib.ora_integrate_ray_stream_counted(cpu._h, C.byref(ray), C.c_int32(method), *args, C.c_uint64(m), C.c_uint32(1), counted,
                                                              C.c_uint64(0), C.c_uint64(0), C.byref(rays)))
                O._check(lib.ora_integrate_ray_stream_counted(cpu._h, C.byref(ray), C.c_int32(method), *args, C.c_uint64(m), C.c_uint32(1), quiet,
                                                              C.c_uint64(0), C.c_uint64(0), None))  # (the count is optional)
                assert bytes(old) == bytes(stream) == bytes(counted) == bytes(quiet)
                mean, n = cpu.integrate_ray(o[i], d[i], method, m, seed=5, n_threads=1, return_rays=True)
                assert mean.tobytes() == bytes(counted) and n == rays.value  # written, not added to
                assert cpu.integrate_ray(o[i], d[i], method, m, seed=5, n_threads=1).tobytes() == mean.tobytes()
                # summed over the samples, however the samples are split over threads
                singles = [cpu.integrate_ray(o[i], d[i], method, 1, seed=5, n_threads=1, sample_begin=k, return_rays=True)[1] for k in range(m)]
                assert n == sum(singles) == cpu.integrate_ray(o[i], d[i], method, m, seed=5, n_threads=2, return_rays=True)[1]


def test_ray_counts_on_the_view_of_the_sky():
    """the answer test_gpu_lens.py's test_ray_counters_on_a_view_of_the_sky already knows: 1 per naive sample, 0 per MIS sample (the
    prologue's exit lies ahead of the first sample_lights call), 0 per black sample"""
    import importlib
    hb = importlib.import_module("raytracing-rust_amd.hip_backend")
    cpu = LN.built("rtweekend1")[2]
    for projection in LN.SKY_ONLY_PROJECTIONS:
        cam = LN.camera(hb, "rtweekend1", projection, params=LN.SKY_ONLY_CAMERA)
        for method, each in ((NAIVE, 1), (MIS, 0)):
            img, inside, rays = LC.pass_image(cpu, cam, LN.W, LN.H, method, LN.SEED, LN.BEGIN, return_rays=True)
            assert rays.dtype == np.uint64 and (rays == np.where(inside, each, 0)).all(), (projection, method)
            assert (inside.all()) == (projection != "fisheye") and inside.any()
            two = LC.pass_image(cpu, cam, LN.W, LN.H, method, LN.SEED, LN.BEGIN)  # the existing callers' two values, the same bytes
            assert len(two) == 2 and two[0].tobytes() == img.tobytes() and two[1].tobytes() == inside.tobytes()
        for spp, split in LN.FOLDS:
            assert LN.rays_shot("rtweekend1", NAIVE, projection, spp, sky_only=True) == LN.reference("rtweekend1", NAIVE, projection, spp, split, sky_only=True)[2]
    o = LN.opts(MIS, 4, 2)
    cam = LN.camera(hb, "all_materials", "fisheye")
    f3, f4 = LC.frame(LN.built("all_materials")[2], cam, o, 2), LC.frame(LN.built("all_materials")[2], cam, o, 2, return_rays=True)
    assert len(f3) == 3 and len(f4) == 4 and f3[0].tobytes() == f4[0].tobytes() and f3[2] == f4[2]
    assert f4[3] == LN.rays_shot("all_materials", MIS, "fisheye", 4) > 0 and f4[0].tobytes() == LN.reference("all_materials", MIS, "fisheye", 4, 2)[0].tobytes()


@pytest.mark.parametrize("key", ["streams"] + [f"shape/{n}" for n in RC.SHAPES] + ["sky/control/spheres", "sky/plateaus/lit_spheres"])
def test_ray_counts_obey_the_integrators_bounds(key):
    """From oracle/ora_render.c, for ONE sample at max_depth D:
      ora_naive_get_colour  counts one ray per trip of `while (depth < D)`, depth rises by one per trip and nothing else ends a
                            trip early before the count: 1 <= rays <= D for D >= 1 (exactly 1 when the first ray leaves the scene:
                            the sky's scatter exits), 0 for D = 0;
      ora_mis_get_colour    counts nothing in the prologue and one ray per trip of `while (depth < D)` from depth 1, at the
                            sample_lights call: 0 <= rays <= D - 1, and exactly 0 when D <= 1 or the prologue's scatter exits (the
                            first ray leaves the scene, or meets an emitter); at least 1 otherwise, for D >= 2.
    The fixed-ray entry cannot be tied to Scene.render byte for byte (a camera's draws differ), so the count is pinned by these."""
    cpu = RC.built(key)[2]
    o, d, _ = RC.rays(key)
    o, d = o[::3], d[::3]
    rec = cpu.check_hit(o, d)
    leaves = ~((rec["found"] != 0) & (rec["index"] != NO_INDEX))
    lights = set(int(i) for i in cpu.lights())
    first_is_light = np.array([int(i) in lights for i in rec["index"]]) & ~leaves
    seen = {NAIVE: set(), MIS: set()}
    for depth in (0, 1, 2, 8, 50):
        for i in range(len(o)):
            kw = dict(seed=RC.SEED, max_depth=depth, n_threads=1, stream=i, return_rays=True)
            naive, mis = (cpu.integrate_ray(o[i], d[i], m, 1, **kw)[1] for m in (NAIVE, MIS))
            assert (naive == 0) if depth == 0 else (1 <= naive <= depth), (key, depth, i, naive)
            assert 0 <= mis <= max(depth, 1) - 1, (key, depth, i, mis)
            if leaves[i]:
                assert naive == min(depth, 1) and mis == 0, (key, depth, i)
            elif first_is_light[i]:
                assert mis == 0, (key, depth, i)  # (an emitter's scatter exits: the prologue returns)
            seen[NAIVE].add(naive)
            seen[MIS].add(mis)
    assert len(seen[NAIVE]) >= 3 and len(seen[MIS]) >= 2, (key, seen)  # (the count is no constant)
    if not leaves.all():
        assert max(seen[MIS]) >= 1


# ---- every reference: what it holds, that it repeats, and the ray counts ----
@pytest.mark.parametrize("group", list(LR.GROUPS))
def test_references_hold_and_repeat(group):
    keys = LR.GROUPS[group]
    with_nan = []
    for key in keys:
        e, r = LR.ENTRIES[key], LR.reference(key)
        img, inside, rays = LR.passes(key)
        print(f"{key}: reference holds a NaN: {r.has_nan}; inside samples {r.inside} of {e.w * e.h * e.spp}; rays {r.rays}")
        if r.has_nan:
            with_nan.append(key)
        assert r.frame.shape == (e.h, e.w, 3) and (r.sums is None) == (e.split == 1), key
        assert _same(LR.fold(img, e.split), r.frame, nan_equal=r.has_nan), key  # tiles_cases' fold and lens_checker's agree
        assert r.inside == int(inside.sum()) and r.rays == int(rays.sum()) and (rays[~inside] == 0).all(), key
        assert (img[~inside].view(np.uint32) == 0).all(), key  # a black sample is +0
        assert (r.inside == e.w * e.h * e.spp) == (e.projection != "fisheye"), key
        if e.split > 1:
            assert r.tiled.shape == (e.split, e.n_tiles(), 8, 8, 3) and (r.tiled[:, LR.padding(e.w, e.h)].view(np.uint32) == 0).all(), key
        # MIS counts a ray per sample_lights call, and max_depth 1 leaves through the prologue's exit before the first one
        assert (r.rays == 0) if (e.method == MIS and e.max_depth == 1) else (r.rays > 0), key
        if e.method == NAIVE:
            assert r.inside <= r.rays <= e.max_depth * r.inside, key
        else:
            assert r.rays <= (e.max_depth - 1) * r.inside, key
    for key in keys[::7]:  # computed again, past every cache
        e = LR.ENTRIES[key]
        again = LC.frame(LR.built(e.ref_scene)[2], LR.camera(key), LR.opts(key), e.split, return_rays=True)
        r = LR.reference(key)
        assert again[0].tobytes() == r.frame.tobytes() and again[2:] == (r.inside, r.rays), key
        assert (again[1] is None and r.sums is None) or again[1].tobytes() == r.sums.tobytes(), key
    print(f"{group}: {len(keys)} entries; the reference frame holds a NaN in {with_nan or 'none'}")
    if group != "depth":  # the d1 MIS references are where a NaN is allowed, if anywhere
        assert not with_nan
    else:
        assert all(LR.ENTRIES[k].method == MIS and LR.ENTRIES[k].max_depth == 1 for k in with_nan)


# ---- 1. skies ----
def _table_rows(dirs, res_y):
    """the row of the sky's table a direction falls in: Sky::pdf's v = acos(z) / pi of the unit vector, times res_y"""
    d = dirs.astype(np.float64)
    z = d[:, 2] / np.linalg.norm(d, axis=1)
    return np.minimum((np.arccos(np.clip(z, -1.0, 1.0)) / np.pi * res_y).astype(np.int64), res_y - 1)


@pytest.mark.parametrize("key", [k for k in LR.SKIES if "/mis" in k])
def test_sky_entry_reaches_the_sampler_and_the_tables_polar_rows(hb, key):
    _, case, scene = key.split("/")[:3]
    e = LR.ENTRIES[key]
    if case not in SK.HUGE:  # (a host build of a 2^24-cell table: test_sky_tables.py does it once)
        si = hb.HipScene(LR.built(e.scene)[0], device=abi.RT_DEVICE_NONE).sky_info()
        assert (si["res_x"], si["res_y"]) == tuple(SK.CASES[case].res) and si["guide_k"] == SK.CASES[case].guide_k, key
        assert si["inv_res_ok"] == SK.CASES[case].inv_res_ok
    assert (e.w, e.h, e.spp, e.split) == ((8, 16, 2, 2) if case in SK.HUGE else (16, 16, 4, 2))
    cam = LR.camera(key)
    assert np.array(cam.up[:], F32).tobytes() == np.array([0, 0, 1], F32).tobytes()  # the level camera: `up` is the table's pole
    frame = LR.reference(key).frame
    # the same scene under `control` (for `control` itself: under the same texture, never sampled), and under NAIVE
    other = f"unsampled/{case}/{scene}" if case == "control" else f"sky/control/{scene}"
    against = LR.fold(LR.passes(key, scene=other)[0], e.split)
    naive = LR.fold(LR.passes(key, scene=f"unsampled/{case}/{scene}", method=NAIVE)[0], e.split)
    counts = int(_differ(frame, against).sum()), int(_differ(frame, naive).sum())
    print(f"{key}: of {e.w * e.h} pixels {counts[0]} differ from {other}, {counts[1]} from NAIVE")
    assert np.isfinite(frame).all(), key
    if case == "black" and scene != "lit_spheres":
        # (test_tiles_cases.py says why: the sky is the only emitter and its texture is 0, every frame is exactly 0; what the GPU
        # must reproduce is the integrators' NaN filter.  It still differs from `control`, whose sky shines)
        assert (frame == 0).all() and counts[0] >= 1 and counts[1] == 0
    else:
        assert counts[0] >= 1 and counts[1] >= 1, (key, counts)
    if e.projection == "equirect":
        res_y = SK.CASES[case].res[1]
        top, bottom = set(), set()
        for n in LR.pass_indices(e.begin, e.spp):
            _, d, _ = LR.directions(key, n)
            rows = _table_rows(d, res_y).reshape(e.h, e.w)
            top |= set(rows[0].tolist())
            bottom |= set(rows[-1].tolist())
        print(f"{key}: the top pixel row reaches table rows {min(top)}..{max(top)}, the bottom one {min(bottom)}..{max(bottom)} of {res_y}")
        assert 0 in top and res_y - 1 in bottom, (key, sorted(top)[:3], sorted(bottom)[-3:])


@pytest.mark.parametrize("key", [k for k in LR.SKIES if "/naive" in k])
def test_naive_under_a_sampled_sky_is_naive_without_the_sampler(key):
    """the reference of a NAIVE entry is the oracle on SK.unsampled; on the oracle the sampled scene gives the same bytes and rays"""
    e = LR.ENTRIES[key]
    assert e.ref_scene == "unsampled/" + e.scene.split("/", 1)[1]
    img, _, rays = LR.passes(key, scene=e.scene)
    assert LR.fold(img, e.split).tobytes() == LR.reference(key).frame.tobytes() and int(rays.sum()) == LR.reference(key).rays, key


# ---- 2. the four arms of sample_lights ----
def test_the_four_arms_differ_and_nothing_counts_as_naive_does(hb):
    for name in RC.SHAPES:
        host = hb.HipScene(LR.built(f"shape/{name}")[0], device=abi.RT_DEVICE_NONE)
        si = host.sky_info()
        assert (host.counts()[2] > 0, (si["res_x"] | si["res_y"]) != 0) == RC.SHAPES[name][0], name
    for split in (1, 2):
        frames = {n: LR.reference(f"arm/{n}/mis/s{split}").frame for n in RC.SHAPES}
        for a, b in itertools.combinations(RC.SHAPES, 2):
            assert _differ(frames[a], frames[b]).any(), (a, b, split)
        for n in RC.SHAPES:  # and the MIS entries are not the NAIVE ones again
            assert _differ(frames[n], LR.reference(f"arm/{n}/naive/s{split}").frame).any(), n
    # `nothing` is one flat floor under a sky that cannot be sampled: a path is camera -> sky or camera -> floor -> sky (a direction
    # scattered off z = 0 cannot meet z = 0 again).  NAIVE counts its check_hit calls, 1 or 2; MIS counts its sample_lights calls,
    # none in the prologue and one at the floor, 0 or 1.  The two integrators draw differently (MIS scatters a clone first), but
    # the ray and so the first hit is the camera's, the same for both: sample by sample NAIVE's count is MIS' plus one.
    _, inside, naive = LR.passes("arm/nothing/naive/s1")
    _, _, mis = LR.passes("arm/nothing/mis/s1")
    assert inside.all() and (naive == mis + np.uint64(1)).all() and set(np.unique(mis).tolist()) == {0, 1}
    assert LR.reference("arm/nothing/naive/s2").rays == LR.reference("arm/nothing/mis/s2").rays + inside.size
    # (on the arms that do sample, the two counts are not tied like this)
    assert not (LR.passes("arm/primitives_and_sky/naive/s1")[2] == LR.passes("arm/primitives_and_sky/mis/s1")[2] + np.uint64(1)).all()


# ---- 3. uneven chunks ----
@pytest.mark.parametrize("key", LR.UNEVENS)
def test_uneven_split_shows_its_chunk_rule(key):
    e = LR.ENTRIES[key]
    b, alt = N.chunk_bounds(e.spp, e.split), TC.ceil_bounds(e.spp, e.split)
    lengths = [hi - lo for lo, hi in zip(b, b[1:])]
    img, inside, _ = LR.passes(key)
    frame = LR.reference(key).frame
    running, other = int(_differ(frame, LR.fold(img, 1)).sum()), int(_differ(frame, LR.fold(img, e.split, alt)).sum())
    print(f"{key}: chunks {lengths}; of {e.w * e.h} pixels {running} differ from the split-1 fold, {other} from the ceil rule")
    assert running >= 1, key
    if e.split == e.spp:  # chunks of one pass under either rule: no frame can tell them apart; these entries end a chunk at EVERY pass
        assert alt == b and other == 0 and set(lengths) == {1}, key
    else:
        assert alt != b and other >= 1 and len(set(lengths)) > 1, key
        assert _differ(N.chunk_sums(img, e.split)[0], N.chunk_sums(img, e.split, alt)[0]).any(), key
    # pixels with black and drawn samples inside one chunk, and pixels all of whose samples are black (the fisheye's corners)
    assert (~inside.any(axis=0)).any() and (inside.any(axis=0) & ~inside.all(axis=0)).any(), key


# ---- 4. 64-bit seeds and first samples, on both streams ----
@pytest.mark.parametrize("key", LR.STREAMS)
def test_a_dropped_high_word_changes_more_than_half_of_the_frame(key):
    e = LR.ENTRIES[key]
    frame = LR.reference(key).frame
    idx = LR.pass_indices(e.begin, e.spp)
    half, shown = e.w * e.h // 2, []
    if e.seed > LR.LOW:
        n = int(_differ(frame, LR.fold(LR.passes(key, seed=e.seed & LR.LOW)[0], e.split)).sum())
        assert n > half, (key, "seed", n)
        shown.append(f"seed cut: {n}")
    cut = [((e.begin & LR.LOW) + k) & LR.LOW for k in range(e.spp)]  # sample_begin + k in 32 bits
    assert cut != idx
    n = int(_differ(frame, LR.fold(LR.passes(key, indices=cut)[0], e.split)).sum())
    assert n > half, (key, "first sample cut", n)
    shown.append(f"first sample cut: {n}")
    no_carry = [(e.begin & ~LR.LOW & LR.MASK64) | ((e.begin + k) & LR.LOW) for k in range(e.spp)]  # the low words added, the high word kept
    if no_carry != idx:
        first = next(k for k in range(e.spp) if no_carry[k] != idx[k])
        assert first >= 1 and (idx[first] & LR.LOW) == 0, key  # the pass the carry (or the wrap) produces
        n = int(_differ(frame, LR.fold(LR.passes(key, indices=no_carry)[0], e.split)).sum())
        assert n > half, (key, "no carry", n)
        shown.append(f"no carry, from pass {first}: {n}")
    else:
        assert e.begin == 1 << 32  # the one first sample whose passes do not carry
    print(f"{key}: of {e.w * e.h} pixels -- " + "; ".join(shown))


def test_the_wrap_and_the_camera_stream(O):
    for method in ("naive", "mis"):
        key = f"stream/{method}/s2/{RC.SEEDS[2]:#x}/{(1 << 64) - 2:#x}"
        e = LR.ENTRIES[key]
        img, inside, rays = LR.passes(key)
        # the third pass of the frame from 2^64 - 2 is the pass at sample 0: the checker handed the unwrapped sum, and sample 0 itself
        unwrapped = LC.pass_image(LR.built(e.ref_scene)[2], LR.camera(key), e.w, e.h, e.method, e.seed, e.begin + 2, return_rays=True)
        zero = LR.single_pass(e.ref_scene, e.scene, e.method, e.projection, e.aperture, e.camera, e.w, e.h, e.seed, 0)
        assert e.begin + 2 == 1 << 64 and img[2].tobytes() == unwrapped[0].tobytes() == zero[0].tobytes()
        assert rays[2].tobytes() == unwrapped[2].tobytes() == zero[2].tobytes()
        other = LR.single_pass(e.ref_scene, e.scene, e.method, e.projection, e.aperture, e.camera, e.w, e.h, e.seed, 1 << 32)
        assert _differ(img[2], other[0]).mean() > 0.5
    # the camera's draws are those of the stream 2^63 + pixel, not of the path's stream `pixel`, at every seed and first sample
    for seed in RC.SEEDS:
        for begin in LR.STREAM_BEGINS:
            draws = LC.camera_draws(seed, 16, 8, begin)
            path = np.stack([O.rng_f32(seed, p, begin, 4) for p in range(16 * 8)])
            assert draws.shape == path.shape == (128, 4) and (draws != path).any(axis=1).all()
            low = np.stack([O.rng_f32(seed, (LC.CAMERA_STREAM + p) & LR.LOW, begin, 4) for p in range(16 * 8)])
            assert low.tobytes() == path.tobytes()  # (what dropping the stream's high word would draw)
    # and all four are used: another lens draw moves more than half of the origins
    key = LR.STREAMS[0]
    o, _, _ = LR.directions(key)
    assert (np.unique(o, axis=0).shape[0]) > 64


# ---- 5. depth and roulette ----
@pytest.mark.parametrize("scene", LR.DEPTH_SCENES)
@pytest.mark.parametrize("method", ["naive", "mis"])
def test_depth_and_roulette_frames_differ_pairwise(scene, method):
    keys = [f"depth/{scene}/{method}/d{d}/r{r}" for d in LR.DEPTHS for r in LR.ROULETTES]
    for a, b in itertools.combinations(keys, 2):
        n = int(_differ(LR.reference(a).frame, LR.reference(b).frame).sum())
        print(f"{a} against {b}: {n} of 128 pixels differ")
        da, db = a.split("/")[3], b.split("/")[3]
        if da == db and da in ("d1", "d2"):
            # Two of the fifteen pairs are the same bytes by the integrators' own definition, as test_tiles_cases.py derives:
            # roulette is played at a vertex when `depth > rr_threshold`, the first vertex (depth 0) never plays, and at
            # max_depth 2 the only vertex that can (depth 1) is the path's last, so neither survival nor the rescaled throughput
            # reaches anything.  rr_threshold cannot show below max_depth 3; d2/r0 stays, as the entry at which `>=` in place
            # of `>` would play at the FIRST vertex.  The ray counts are the same too.
            assert n == 0 and LR.reference(a).frame.tobytes() == LR.reference(b).frame.tobytes() and LR.reference(a).rays == LR.reference(b).rays
        else:
            assert n >= 1, (a, b)
    for key in keys:
        assert (LR.reference(key).frame != 0).any(), key
    # the ray counts tell the depths apart as well: at most inside x depth (NAIVE), inside x (depth - 1) (MIS), and growing
    counts = [LR.reference(f"depth/{scene}/{method}/d{d}/r3").rays for d in LR.DEPTHS]
    assert counts[0] < counts[1] < counts[2], counts
    assert counts[0] == (128 * 4 if method == "naive" else 0)


# ---- 6. ragged frames ----
def test_ragged_frames_divide_the_jitter_by_one_and_fill_their_tiles_unevenly():
    for key in LR.RAGGEDS:
        e = LR.ENTRIES[key]
        assert LR.padding(e.w, e.h).sum() == 64 * e.n_tiles() - e.w * e.h
        assert np.unique(LR.reference(key).frame.reshape(-1, 3), axis=0).shape[0] >= 2, key  # a frame, not a constant
    # at 2 x 2, s = jitter + x: the samples of pixel column 1 lie at s in [1, 2), beyond the viewport's edge
    for p in abi.PROJECTIONS:
        key = f"ragged/2x2/{p}/s1"
        d = LC.camera_draws(LR.SEED, 2, 2, LR.BEGIN)
        s = (LC.jitter_from_f32(d[:, 0]) + np.array([0, 1, 0, 1], F32)) / F32(1)
        assert (s[[1, 3]] >= 1).all() and (s[[0, 2]] < 1).all()
        assert np.isfinite(LR.directions(key)[1][LR.directions(key)[2]]).all()


# ---- 7. cameras ----
def _theta(key):
    """per pass: the angle between each inside sample's direction and `forward`, and the inside mask"""
    e = LR.ENTRIES[key]
    fwd = np.array(LR.camera(key).forward[:], np.float64)
    out = []
    for n in LR.pass_indices(e.begin, e.spp):
        _, d, inside = LR.directions(key, n)
        d = d.astype(np.float64)
        cos = (d @ fwd) / np.linalg.norm(d, axis=1)
        out.append((np.arccos(np.clip(cos, -1, 1)), inside))
    return np.stack([t for t, _ in out]), np.stack([i for _, i in out])


@pytest.mark.parametrize("fov", LR.WIDE_FOVS)
def test_the_wide_fisheye_looks_backwards(fov):
    for method in ("naive", "mis"):
        key = f"camera/fisheye{fov:.0f}/{method}"
        e = LR.ENTRIES[key]
        theta, inside = _theta(key)
        behind = (theta[inside] > np.pi / 2).mean()
        share = inside.mean()
        print(f"{key}: {share:.3f} of the samples inside, {behind:.3f} of them with theta > pi/2, the largest theta {theta[inside].max():.3f}")
        assert behind >= 0.1, key
        assert 0.5 < share < 0.95 and LR.reference(key).inside == int(inside.sum()), key
        assert abs(float(LR.camera(key).fisheye_half_angle) - np.radians(fov) / 2) < 1e-6
        if fov == 360.0:
            assert (theta[inside] > np.pi - 0.2).any(), key  # within 0.2 rad of -forward
        # the frame is not the scene's own fisheye's
        own = LR.single_pass(e.ref_scene, e.scene, e.method, "fisheye", 0.0, (), e.w, e.h, e.seed, e.begin)
        assert _differ(LR.passes(key)[0][0], own[0]).mean() > 0.5


def test_the_fisheye_on_frames_far_from_square():
    """24 x 8: b = (2 t - 1) * 7 / 23 stays within +-7/23, so the image circle is cut by the frame's top and bottom; s = (x + jitter)
    / 23 reaches 1 at the last pixel column, whose samples all have a >= 1 with b != 0: that column is entirely black -- lanes all
    of whose passes go START -> FINISH -- while the centre columns are entirely inside.  The transposed frame, 8 x 24, scales b
    by 23 / 7: whole pixel ROWS are black above and below the circle, and the last column as well."""
    for method in ("naive", "mis"):
        _, inside, rays = LR.passes(f"camera/fisheye_24x8/{method}")
        black_columns = (~inside).all(axis=(0, 1))
        assert inside.shape == (4, 8, 24) and black_columns[23] and black_columns.sum() >= 1
        assert inside[:, :, 11:13].all() and inside[:, :, 1:22].all()  # the centre columns, and all but the frame's ends
        assert (rays[:, :, black_columns] == 0).all() and 0.9 < inside.mean() < 1.0
        assert (LR.reference(f"camera/fisheye_24x8/{method}").frame[:, black_columns].view(np.uint32) == 0).all()
        _, inside, rays = LR.passes(f"camera/fisheye_8x24/{method}")
        rows_black = (~inside).all(axis=(0, 2))
        assert inside.shape == (4, 24, 8) and rows_black[:8].all() and rows_black[15:].all() and not rows_black[8:15].any()
        assert inside[:, 10:13, 1:6].all() and (~inside)[:, :, 7].all() and (rays[:, rows_black] == 0).all()
        assert (LR.reference(f"camera/fisheye_8x24/{method}").frame[rows_black].view(np.uint32) == 0).all()


def test_the_big_lens_starts_rays_inside_the_ground():
    """primitive 0 of scenes.all_materials() is the ground, a sphere of radius 1000 about (0, -1000, 0): an origin is inside it
    when its distance from that centre is below 1000"""
    centre = np.array(LR.GROUND_CENTRE, np.float64)
    for method in ("naive", "mis"):
        key = f"camera/big_lens/{method}"
        e = LR.ENTRIES[key]
        cam, params = LR.camera(key), LR.built(e.scene)[1]
        assert float(cam.lens_radius) == 4.0 and dict(e.camera)["focus_dist"] not in (1.0, params["focus_dist"])
        height = np.linalg.norm(np.array(params["origin"], np.float64) - centre) - LR.GROUND_RADIUS
        assert 1.0 < height < float(cam.lens_radius)  # the lens reaches past the nearest object
        small = LR.ENTRIES["arm/nothing/mis/s1"].aperture / 2
        assert small < height
        for n in LR.pass_indices(e.begin, e.spp):
            o, d, inside = LR.directions(key, n)
            below = np.linalg.norm(o.astype(np.float64) - centre, axis=1) < LR.GROUND_RADIUS
            assert inside.all() and below.sum() >= 1 and (~below).sum() >= 1, (key, n)
        sc = LR.built(e.scene)[0].desc()
        assert sc.n_primitives >= 1
        # the frame is neither the pinhole's nor the small lens'
        pin = LR.single_pass(e.ref_scene, e.scene, e.method, "perspective", 0.0, e.camera, e.w, e.h, e.seed, e.begin)
        lens = LR.single_pass(e.ref_scene, e.scene, e.method, "perspective", LR.APERTURE, e.camera, e.w, e.h, e.seed, e.begin)
        first = LR.passes(key)[0][0]
        assert _differ(first, pin[0]).mean() > 0.5 and _differ(first, lens[0]).mean() > 0.5


def test_a_tilted_vup_tilts_the_basis():
    for p in ("equirect", "orthographic"):
        for method in ("naive", "mis"):
            key = f"camera/tilted_{p}/{method}"
            e = LR.ENTRIES[key]
            cam = LR.camera(key)
            right, up = np.array(cam.right[:], F32), np.array(cam.up[:], F32)
            assert (right != 0).all() and (up != 0).all()  # no component of the basis is zero: every term of the direction's sum counts
            own = LR.single_pass(e.ref_scene, e.scene, e.method, p, 0.0, (), e.w, e.h, e.seed, e.begin)
            assert _differ(LR.passes(key)[0][0], own[0]).mean() > 0.5, key
