"""The tile-render table (tests/tiles_cases.py) on the CPU, oracle only: every entry is in the regime it is there for and its
reference can show the property it is there for, before any GPU is involved -- a sky whose MIS frame equalled the unsampled one
would never reach sample_lights, an uneven split whose frame equalled that of another chunk rule would let the kernel use that
rule, a 64-bit first sample whose frame equalled that of its low word would let the kernel drop the high word.  No entry is
skipped: where an entry provably cannot show a property, the reason is stated and the exact property it has instead is asserted.
Every reference is also rebuilt from the oracle's single passes by noise_checker's fold, so the chunk rule of the checker
(chunk_bounds) is held to the oracle's."""
import itertools

import numpy as np
import pytest

import noise_checker as N
import radiance_cases as RC
import scenes
import sky_cases as SK
import tiles_cases as TC

abi = scenes.abi
F32 = np.float32


def _same(a, b, nan_equal=False):
    same = a.view(np.uint32) == b.view(np.uint32)
    if nan_equal:
        same = same | (np.isnan(a) & np.isnan(b))
    return bool(same.all())


def _differs(a, b, m):
    """how many listed pixels differ in any channel (NaN against NaN does not count)"""
    d = ((a != b) & ~(np.isnan(a) & np.isnan(b))).any(axis=-1)
    return int((d & m).sum())


# ---- the table itself ----
def test_the_table_has_the_groups_the_kernel_needs():
    assert len(SK.RENDER_CASES) == 14 and len(SK.HUGE) == 2
    assert len(TC.SKIES) == 12 * 4 + 2 * 2 and len(TC.ARMS) == 16 and len(TC.UNEVENS) == 12
    assert len(TC.STREAMS) == 2 * 2 * 3 * 4 and len(TC.DEPTH_KEYS) == 2 * 2 * 6 and len(TC.RAGGEDS) == 10
    assert len(TC.ENTRIES) == sum(map(len, (TC.SKIES, TC.ARMS, TC.UNEVENS, TC.STREAMS, TC.DEPTH_KEYS, TC.RAGGEDS)))
    for case in SK.RENDER_CASES:
        got = sorted(k.split("/", 2)[2] for k in TC.SKIES if k.split("/")[1] == case)
        assert got == (["floor/mis", "floor/naive"] if case in SK.HUGE else ["floor/mis", "floor/naive", "lit_spheres/mis", "spheres/mis"]), case
    for key, e in TC.ENTRIES.items():
        assert e.w >= 2 and e.h >= 2 and 1 <= e.split <= e.spp, key
        for tiles in e.lists:
            assert len(tiles) >= 1 and all(a > b for a, b in zip(tiles, tiles[1:])) and max(tiles) < e.n_tiles(), (key, tiles)
            # a proper subset -- but for the one frame that has a single tile
            assert len(tiles) < e.n_tiles() or (e.w, e.h) == (2, 2), (key, tiles)
        assert TC.listed(key).any() and ((~TC.listed(key)).any() or (e.w, e.h) == (2, 2)), key
    for key in TC.ARMS:  # the second list is the complement of the first
        e = TC.ENTRIES[key]
        assert sorted(e.lists[0] + e.lists[1]) == list(range(e.n_tiles()))
    assert [TC.ENTRIES[k].groups for k in TC.UNEVENS].count((0, 1)) == 2  # one (spp, S), both methods
    # 64-bit first samples: the carry inside the passes and on the chunk boundary of split 2, and the wrap
    assert TC.pass_indices((1 << 32) - 2, 4) == [(1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]
    assert N.chunk_bounds(4, 2)[1] == 2  # pass 2 of 2^32 - 2 is 2^32: the first pass of the second chunk
    assert TC.pass_indices((1 << 64) - 2, 4) == [(1 << 64) - 2, (1 << 64) - 1, 0, 1]
    ragged = {(TC.ENTRIES[k].w, TC.ENTRIES[k].h) for k in TC.RAGGEDS}
    assert ragged == {(2, 2), (5, 11), (9, 8)}


# ---- the checker's chunk rule ----
def _equal_chunk_sums(pass_images, split):
    """chunk_sums as it was when it took dividing splits only"""
    n = len(pass_images) // split
    sums = np.zeros((split,) + pass_images.shape[1:], F32)
    for c in range(split):
        for s in range(c * n, (c + 1) * n):
            sums[c] = sums[c] + pass_images[s]
    return sums


def test_chunk_bounds_are_the_equal_chunks_where_the_split_divides_and_the_headers_floors_elsewhere():
    rng = np.random.default_rng(3)
    for spp in range(1, 17):
        images = (rng.random((spp, 3, 5, 3), dtype=np.float32) * F32(1e3)).astype(F32)
        for split in range(1, spp + 1):
            b = N.chunk_bounds(spp, split)
            assert len(b) == split + 1 and b[0] == 0 and b[-1] == spp and all(lo < hi for lo, hi in zip(b, b[1:])), (spp, split)
            assert b == [int(np.floor(c * spp / split)) for c in range(split + 1)]
            if spp % split == 0:
                assert b == [c * (spp // split) for c in range(split + 1)]
                assert N.chunk_sums(images, split).tobytes() == _equal_chunk_sums(images, split).tobytes(), (spp, split)
    with pytest.raises(AssertionError):  # the noise estimates still require equal chunks
        N.estimate(N.chunk_sums(np.zeros((7, 2, 2, 3), F32), 3), 7)


def _kernel_chunks(spp, split, floor_j=False):
    """tiles_kernel's whole-pixel item, its chunk rule alone: the chunk ends it folds at, or None if the pixel never finishes.
    R_CHUNK_END starts at floor(spp / S); at a chunk's end k the next chunk is j = ceil(k S / spp) and ends at floor((j + 1) spp / S)"""
    end, ends = spp // split, []
    for k in range(1, spp + 1):
        if k == end:
            ends.append(k)
            j = (k * split) // spp if floor_j else (k * split + spp - 1) // spp
            if k == spp:
                return ends
            end = ((j + 1) * spp) // split
    return None


def test_the_kernels_chunk_rule_is_the_headers_and_a_floor_in_it_never_finishes_an_uneven_pixel():
    """why the mutation `j computed with floor` is shown here and not run on a GPU: by this arithmetic the pixel's chunk end falls
    back on the pass just folded and is never met again -- the kernel would not end"""
    for spp in range(1, 33):
        for split in range(1, spp + 1):
            assert _kernel_chunks(spp, split) == N.chunk_bounds(spp, split)[1:], (spp, split)
    for spp, split in TC.UNEVEN:
        if split == spp:  # chunks of one pass: k S / spp is an integer, floor and ceil agree
            assert _kernel_chunks(spp, split, floor_j=True) == N.chunk_bounds(spp, split)[1:]
        else:
            assert _kernel_chunks(spp, split, floor_j=True) is None, (spp, split)
    assert _kernel_chunks(8, 4, floor_j=True) == [2, 4, 6, 8]  # (a dividing split, all the older tests have, cannot tell)


# ---- every reference: repeats, and is the checker's fold of the oracle's single passes ----
@pytest.mark.parametrize("group", ["sky", "arm", "uneven", "stream", "depth", "ragged"])
def test_references_repeat_and_are_the_fold_of_their_passes(group):
    keys = [k for k in TC.ENTRIES if k.startswith(group + "/")]
    with_nan = []
    for key in keys:
        e = TC.ENTRIES[key]
        frame, rays = TC.reference(key)
        nan = TC.has_nan(key)
        if nan:
            with_nan.append(key)
        assert _same(TC.fold(TC.passes(key), e.split), frame, nan_equal=nan), key
        # (MIS counts a ray per sample_lights call, and max_depth 1 leaves through the prologue's exit before the first one)
        assert (rays == 0) if (e.method == TC.MIS and e.max_depth == 1) else (rays > 0), key
    for key in keys[::7]:
        again, rays = TC.render(TC.ENTRIES[key].ref_scene, TC.opts(key))
        assert again.tobytes() == TC.reference(key)[0].tobytes() and rays == TC.reference(key)[1], key
    print(f"{group}: {len(keys)} entries; the oracle frame holds a NaN in {with_nan or 'none'}")


# ---- 1. skies ----
@pytest.mark.parametrize("key", [k for k in TC.SKIES if k.endswith("/mis")])
def test_sky_entry_reaches_the_sampler(hb, key):
    _, case, scene, _ = key.split("/")
    e = TC.ENTRIES[key]
    sc = TC.built(e.scene)[0]
    if case not in SK.HUGE:  # (a host build of a 2^24-cell table: test_sky_tables.py does it once, for the same texture and resolution)
        host = hb.HipScene(sc, device=abi.RT_DEVICE_NONE)
        si = host.sky_info()
        assert (si["res_x"], si["res_y"]) == tuple(SK.CASES[case].res) and si["guide_k"] == SK.CASES[case].guide_k, key
        assert si["inv_res_ok"] == SK.CASES[case].inv_res_ok
        assert (host.counts()[2] > 0) == (scene == "lit_spheres")
    assert (e.w, e.h, e.spp, e.split, e.lists) == ((8, 16, 2, 2, ((1,),)) if case in SK.HUGE else (16, 16, 4, 2, ((3, 0),)))
    m = TC.listed(key)
    mis = TC.reference(key)[0]
    o = TC.opts(key)
    plain_mis = TC.render(f"unsampled/{case}/{scene}", o)[0]  # the same texture, never sampled
    o.render_method = TC.NAIVE
    plain_naive = TC.render(f"unsampled/{case}/{scene}", o)[0]
    counts = _differs(mis, plain_mis, m), _differs(mis, plain_naive, m)
    print(f"{key}: of {int(m.sum())} listed pixels MIS differs from MIS without a sampler on {counts[0]}, from NAIVE on {counts[1]}; "
          f"non-zero on {int(((mis != 0).any(axis=-1) & m).sum())}")
    assert np.isfinite(mis).all(), key
    if case == "black" and scene != "lit_spheres":
        # test_radiance_cases.py exempts the same entries for the same reason: the sky is the only emitter and its texture is 0, so
        # every emission term is +0 and a light sample's `eval * weight * 0 / l_pdf` with l_pdf == 0 is NaN, filtered to 0
        # (mis.rs:88-90).  The frame is exactly 0 under either integrator; what the GPU must reproduce here is the filter.
        assert (mis == 0).all() and (plain_naive == 0).all() and counts == (0, 0)
        return
    assert counts[0] >= 1 and counts[1] >= 1, (key, counts)


@pytest.mark.parametrize("key", [k for k in TC.SKIES if k.endswith("/naive")])
def test_naive_under_a_sampled_sky_is_naive_without_the_sampler(key):
    """the reference of a NAIVE entry is the oracle on SK.unsampled; on the oracle the sampled scene gives the same bytes"""
    e = TC.ENTRIES[key]
    assert e.ref_scene == "unsampled/" + e.scene.split("/", 1)[1]
    sampled, rays = TC.render(e.scene, TC.opts(key))
    assert sampled.tobytes() == TC.reference(key)[0].tobytes() and rays == TC.reference(key)[1], key


# ---- 2. the four arms of sample_lights ----
@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_arm_flags_read_from_the_scene(hb, name):
    host = hb.HipScene(TC.built(f"shape/{name}")[0], device=abi.RT_DEVICE_NONE)
    si = host.sky_info()
    shape = (host.counts()[2] > 0, (si["res_x"] | si["res_y"]) != 0)  # (csrc/rt_shade.h sky_can_sample)
    assert shape == RC.SHAPES[name][0], (name, shape)
    keys = [k for k in TC.ARMS if k.split("/")[1] == name]
    assert len(keys) == 4
    for key in keys:
        e = TC.ENTRIES[key]
        frame, rays = TC.reference(key)
        assert np.isfinite(frame).all() and (frame[TC.listed(key)] != 0).any() and rays > 0, key
    for split in (1, 2):  # the two integrators do not agree on the listed pixels: the MIS entries are not the NAIVE ones again
        a, b = (TC.reference(f"arm/{name}/{m}/s{split}")[0] for m in ("naive", "mis"))
        assert _differs(a, b, TC.listed(f"arm/{name}/mis/s{split}")) >= 1, (name, split)
    assert {RC.SHAPES[n][0] for n in RC.SHAPES} == {(False, True), (False, False), (True, False), (True, True)}


# ---- 3. uneven chunks ----
@pytest.mark.parametrize("key", TC.UNEVENS)
def test_uneven_split_shows_its_chunk_rule(key):
    e = TC.ENTRIES[key]
    spp, split = e.spp, e.split
    b = N.chunk_bounds(spp, split)
    lengths = [hi - lo for lo, hi in zip(b, b[1:])]
    alt = TC.ceil_bounds(spp, split)
    m = TC.listed(key)
    frame = TC.reference(key)[0]
    p = TC.passes(key)
    running = _differs(frame, TC.fold(p, 1), m)
    other = _differs(frame, TC.fold(p, split, alt), m)
    print(f"{key}: chunks {lengths}, the alternative {[hi - lo for lo, hi in zip(alt, alt[1:])]}; of {int(m.sum())} listed pixels "
          f"{running} differ from the split-1 fold, {other} from the alternative rule")
    assert running >= 1, key
    if split == spp:
        # chunks of one pass each under either rule (ceil(spp / S) = 1): the two rules are the same bounds, so no frame can tell
        # them apart; what these two entries have that no other has is a chunk end at EVERY pass
        assert len(set(lengths)) == 1 and alt == b and other == 0, key
    else:
        assert len(set(lengths)) > 1 and alt != b and other >= 1, (key, lengths)
    # the chunk sums themselves differ from the alternative's, on listed pixels
    if split != spp:
        assert _differs(N.chunk_sums(p, split)[0], N.chunk_sums(p, split, alt)[0], m) >= 1, key


# ---- 4. 64-bit seeds and first samples ----
@pytest.mark.parametrize("key", TC.STREAMS)
def test_a_dropped_high_word_changes_the_frame(key):
    e = TC.ENTRIES[key]
    m = TC.listed(key)
    frame = TC.reference(key)[0]
    idx = TC.pass_indices(e.begin, e.spp)
    shown = []
    if e.seed > TC.LOW:
        n = _differs(frame, TC.fold(TC.passes(key, seed=e.seed & TC.LOW), e.split), m)
        assert n >= 1, (key, "seed")
        shown.append(f"seed cut: {n}")
    cut = [((e.begin & TC.LOW) + k) & TC.LOW for k in range(e.spp)]  # sample_begin + k in 32 bits
    if cut != idx:
        n = _differs(frame, TC.fold(TC.passes(key, indices=cut), e.split), m)
        assert n >= 1, (key, "first sample cut")
        shown.append(f"first sample cut: {n}")
    no_carry = [(e.begin & ~TC.LOW & TC.MASK64) | ((e.begin + k) & TC.LOW) for k in range(e.spp)]  # the low words added, the high word kept
    if no_carry != idx:
        first = next(k for k in range(e.spp) if no_carry[k] != idx[k])
        assert first >= 1 and (idx[first] & TC.LOW) == 0, key  # the pass the carry (or the wrap) produces
        n = _differs(frame, TC.fold(TC.passes(key, indices=no_carry), e.split), m)
        a, b = (TC.single_pass(e.ref_scene, e.method, e.w, e.h, e.seed, i) for i in (idx[first], no_carry[first]))
        assert n >= 1 and _differs(a, b, m) >= 1, (key, "no carry")
        shown.append(f"no carry, from pass {first}: {n}")
    else:
        assert e.begin == 1 << 32  # the one first sample whose passes do not carry
    print(f"{key}: listed pixels that differ -- " + "; ".join(shown))
    assert shown, key


# ---- 5. depth and roulette ----
@pytest.mark.parametrize("scene", TC.DEPTH_SCENES)
@pytest.mark.parametrize("method", ["naive", "mis"])
def test_depth_and_roulette_frames_differ_pairwise(scene, method):
    keys = [f"depth/{scene}/{method}/d{d}/r{r}" for d in TC.DEPTHS for r in TC.ROULETTES]
    m = TC.listed(keys[0])
    for a, b in itertools.combinations(keys, 2):
        n = _differs(TC.reference(a)[0], TC.reference(b)[0], m)
        print(f"{a} against {b}: {n} of {int(m.sum())} listed pixels differ")
        da, db = a.split("/")[3], b.split("/")[3]
        if da == db and da in ("d1", "d2"):
            # Two of the fifteen pairs are provably the same bytes, by the integrators' own definition (integrators/mod.rs:57-70,
            # mis.rs:72-85): roulette is played at a vertex when `depth > rr_threshold`, the depth is raised AFTER it, and a path
            # that the roulette ends and a path that `depth < max_depth` ends return the same sum.  The first vertex has depth 0
            # and never plays (0 > 0 is false); at max_depth 2 the only vertex that can play (depth 1) is the path's last, so
            # whether it survives, and the rescaled throughput, reach nothing.  rr_threshold therefore cannot show below
            # max_depth 3.  The entries stay: d1 pins the depth exits (the MIS prologue's own among them), and d2/r0 is where
            # `depth >= rr_threshold` in place of `>` would play at the FIRST vertex, whose survivors do go on -- see below.
            assert n == 0 and TC.reference(a)[0].tobytes() == TC.reference(b)[0].tobytes()
        else:
            assert n >= 1, (a, b)
    for key in keys:
        assert (TC.reference(key)[0][m] != 0).any(), key
    # `depth >= rr_threshold` is `depth > rr_threshold - 1`: at max_depth 8 the d8/r3 frame differs from the oracle's at
    # rr_threshold 2, so that entry tells the two comparisons apart; and roulette from depth 1 on (r0) matters at max_depth 3
    # already, the smallest depth at which it can
    e = TC.ENTRIES[keys[-1]]
    assert (e.max_depth, e.rr) == (8, 3)
    o = TC.opts(keys[-1])
    o.rr_threshold = 2
    assert _differs(TC.reference(keys[-1])[0], TC.render(e.ref_scene, o)[0], m) >= 1
    o.max_depth, o.rr_threshold = 3, 0
    at3 = TC.render(e.ref_scene, o)[0]
    o.rr_threshold = 3
    assert _differs(at3, TC.render(e.ref_scene, o)[0], m) >= 1
