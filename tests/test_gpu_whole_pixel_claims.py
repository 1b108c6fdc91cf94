"""Whole-pixel claims (RT_TUNE_WHOLE_PIXEL_SHARE, rt_render.hip acquire_coarse): the pair kernels hand the first part of a
shard's tiles out as whole pixels -- a lane folds all S chunks of its pixel, one after the other -- and only the rest chunk by
chunk.  That is HOW work is handed out, never WHAT is computed: every chunk sum is the same sum of the same passes at the same
place of the partial buffer, so frames, ray counts and everything downstream of the partial buffer are the bytes of share 0.

Frames are the smallest on which the hand-out can go wrong: 24 x 16 is six full 8 x 8 tiles (shares 4 and 8 mix both kinds of
claim, 16 is whole-pixel claims only), 19 x 13 is six tiles of which four are edge tiles whose padding lanes ask again at once
and so take part of a LATER claim: the wave then holds leftovers of one claim while it decodes the next.

Leftovers across a change of kind: the tuning interface cannot limit the grid to one workgroup, so no test can force one wave
to walk from whole-pixel claims into chunk claims.  It is argued instead: the kind of a claim travels in the top bit of the
wave's wq_pbase and is copied to old_pbase with the leftovers, and each lane decodes its item by the bit of the claim the item
comes from (`from_old`), never by the kind of the newest claim.  What the cases here do reach is less than that: at 19 x 13 and
share 8 the 40 padding lanes of the last whole-pixel claim (tile 2, three columns wide) ask again with no leftovers in hand and
are served from a chunk claim, which leaves leftovers of CHUNK kind; lanes that finish whole pixels are then served from those.
Leftovers of WHOLE kind next to a newer chunk claim (old_pbase's top bit set, wq_pbase's clear) arise only when a wave takes
fewer than 64 items of a whole-pixel claim, and with far more waves than claims no frame this small makes a wave do that.  That
path needs more claims than waves: the 2560 x 1440 frame of the automatic-share test (one pass per chunk, 18 432 whole-pixel
claims and 39 168 tiles of chunk claims over 6 144 resident waves) runs it, and its bytes are compared with the chunk-only hand-out.

Only the pair kernels (rtweekend1 as the library runs it) are compiled with whole-pixel items.  The general spheres-only kernel
and the triangles-and-lights kernel run the same cases: their launches must report no whole-pixel claim at any share and return
the same bytes -- they share acquire_coarse, whose decode this change rewrote."""
import numpy as np
import pytest

import scenes

abi = scenes.abi
pytestmark = pytest.mark.gpu
TOL = 1e-4  # tests/test_gpu_parity.py: per-channel |delta| < 1e-4 AND bit-identical

FRAMES = ((24, 16), (19, 13))
SPLITS = (4, 16, 64)
SPPS = (64, 70)  # 70: chunks of unequal length (70 / 4, 70 / 16, 70 / 64 leave remainders)
SHARES = (4, 8, 16)


def scene_case(name):
    """(scene description, camera parameters, feature set to force or None)"""
    if name == "rtweekend1_general":  # the same scene on the general spheres-only kernel instead of FeatPair
        ls = scenes.load_ssml("rtweekend1")
        return ls.scene, ls.camera_params, 0
    ls = scenes.load_ssml(name)
    return ls.scene, ls.camera_params, None


def gpu_scene(hb, name):
    sc, cam_params, feature_set = scene_case(name)
    g = hb.HipScene(sc)
    if feature_set is not None:
        g.set_tuning(abi.RT_TUNE_FEATURE_SET, feature_set)
    g.set_tuning(abi.RT_TUNE_SCHEDULE, 0)  # the coarse schedule: the kernels that share acquire_coarse
    return g, hb.camera_new(**cam_params), sc, cam_params


def options(w, h, spp, split, method):
    o = abi.default_render_opts(w, h, spp, method=method, seed=11)
    o.sample_split = split
    return o


def expected_plan(tiles, split, share, name="rtweekend1"):
    whole = tiles * share // 16 if split > 1 and name == "rtweekend1" else 0
    return whole, 64 * (whole + (tiles - whole) * split)


@pytest.mark.parametrize("method", [abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS])
@pytest.mark.parametrize("name", ["rtweekend1", "rtweekend1_general", "overshadowed"])
def test_frames_and_ray_counts_do_not_depend_on_the_share(hb, O, name, method):
    g, cam, sc, cam_params = gpu_scene(hb, name)
    c, ocam = O.Scene(sc), O.camera_new(**cam_params)
    for (w, h) in FRAMES:
        for split in SPLITS:
            for spp in SPPS:
                o = options(w, h, spp, split, method)
                what = f"{name} method {method} {w}x{h} split {split} spp {spp}"
                g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, 0)
                base, base_rays = g.render(cam, o)
                info = g.last_launch_info()
                assert info["fine"] == 0 and info["feature_set"] == {"rtweekend1": 3, "rtweekend1_general": 0}.get(name, info["feature_set"]), (what, info)
                assert (info["whole_claims"], info["n_items"]) == expected_plan(6, split, 0), (what, info)
                ref, ref_rays = c.render(ocam, o)
                assert np.isfinite(base).all() and np.abs(base.astype(np.float64) - ref.astype(np.float64)).max() < TOL, what
                assert np.array_equal(base, ref) and base_rays == ref_rays, what
                for share in SHARES:
                    g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, share)
                    img, rays = g.render(cam, o)
                    info = g.last_launch_info()
                    assert (info["whole_claims"], info["n_items"]) == expected_plan(6, split, share, name), (what, share, info)
                    assert (info["whole_claims"], info["n_items"]) == hb.plan_work_items(o, split, share if name == "rtweekend1" else 0), (what, share, info)
                    assert img.tobytes() == base.tobytes() and rays == base_rays, f"{what} share {share}"


@pytest.mark.parametrize("name", ["rtweekend1", "overshadowed"])
def test_packed_shards_scatter_to_the_unsharded_frame(hb, name):
    """24 x 16 has six tiles: two shards own three each, three own two each, four own 2, 2, 1, 1 -- and a share of a shard's
    tiles rounds down per shard (share 8: 1, 1, 0, 0 whole-pixel claims)"""
    g, cam, _, _ = gpu_scene(hb, name)
    w, h, spp = 24, 16, 70
    for split in (4, 16):
        g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, 0)
        full, full_rays = g.render(cam, options(w, h, spp, split, abi.RT_METHOD_MIS))
        for share in SHARES:
            g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, share)
            for count in (2, 3, 4):
                acc = np.full((w * h, 3), np.nan, dtype=np.float32)
                total = 0
                for idx in range(count):
                    o = options(w, h, spp, split, abi.RT_METHOD_MIS)
                    o.shard_index, o.shard_count, o.output_layout = idx, count, abi.RT_LAYOUT_SHARD
                    part, rays = g.render(cam, o)
                    tiles = (6 - idx + count - 1) // count
                    info = g.last_launch_info()
                    assert (info["whole_claims"], info["n_items"]) == expected_plan(tiles, split, share, name), (split, share, count, idx, info)
                    order = hb.shard_pixel_order(o)
                    valid = order != np.uint64(abi.NO_INDEX)
                    acc[order[valid].astype(np.int64)] = part[valid]
                    total += rays
                assert acc.reshape(h, w, 3).tobytes() == full.tobytes() and total == full_rays, (name, split, share, count)


@pytest.mark.parametrize("name", ["rtweekend1", "overshadowed"])
def test_chunk_sums_are_where_the_later_stages_read_them(hb, name):
    """the partial buffer through the robust stage, which ranks a pixel's S chunk sums and adds the kept ones in chunk order: with
    nothing trimmed (the plain combine), with the median, and the Gini coefficient of the chunk means -- a chunk sum at the wrong
    pixel or under the wrong chunk number changes one of them"""
    g, cam, _, _ = gpu_scene(hb, name)
    for (w, h) in FRAMES:
        for split in SPLITS:
            o = options(w, h, 64, split, abi.RT_METHOD_MIS)  # (the robust stage wants a split that divides the passes)
            g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, 0)
            base = [g.render_robust(cam, o, mode="trim", trim=0), g.render_robust(cam, o, mode="median")]
            plain, _ = g.render(cam, o)
            assert base[0]["out"].tobytes() == plain.tobytes()
            for share in SHARES:
                g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, share)
                got = [g.render_robust(cam, o, mode="trim", trim=0), g.render_robust(cam, o, mode="median")]
                assert g.last_launch_info()["whole_claims"] == (6 * share // 16 if name == "rtweekend1" else 0)
                for a, b in zip(got, base):
                    for channel in ("out", "mean", "gini", "trimmed", "dropped"):
                        assert a[channel].tobytes() == b[channel].tobytes(), (name, w, h, split, share, channel)
                    assert a["rays_shot"] == b["rays_shot"]


def test_the_automatic_share_is_the_default_and_hands_small_frames_out_in_chunks(hb):
    """nobody has set the knob: the planner goes by tiles per resident wave (tests/test_whole_pixel_claims_plan.py restates the
    rule), and the launch reports what the host-side planner says for the device's resident waves; six tiles: no whole claim"""
    g, cam, _, _ = gpu_scene(hb, "rtweekend1")
    for reset in (False, True):
        if reset:
            g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, 16)
            g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, -1)
        o = options(24, 16, 64, 16, abi.RT_METHOD_MIS)
        img, rays = g.render(cam, o)
        info = g.last_launch_info()
        waves = info["n_cus"] * info["blocks_per_cu"] * info["block_threads"] // 64
        assert info["feature_set"] == 3 and (info["whole_claims"], info["n_items"]) == (0, 6 * 64 * 16) == hb.plan_work_items(o, 16, -1, waves), info
    # ... and a frame with many tiles per resident wave at one pass per chunk gets whole claims: the same bytes as without
    o = options(2560, 1440, 16, 16, abi.RT_METHOD_MIS)
    img, rays = g.render(cam, o)
    info = g.last_launch_info()
    waves = info["n_cus"] * info["blocks_per_cu"] * info["block_threads"] // 64
    assert (info["whole_claims"], info["n_items"]) == hb.plan_work_items(o, 16, -1, waves) and info["whole_claims"] > 0, info
    g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, 0)
    base, base_rays = g.render(cam, o)
    assert g.last_launch_info()["whole_claims"] == 0 and img.tobytes() == base.tobytes() and rays == base_rays


def test_the_share_is_checked_and_leaves_other_orders_alone(hb):
    g, cam, _, _ = gpu_scene(hb, "rtweekend1")
    for bad in (-2, 17):
        with pytest.raises(Exception):
            g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, bad)
    g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, 16)
    frames = {}
    for split, tw, th in ((1, 8, 8), (5, 8, 8), (16, 5, 3)):  # S = 1, a split and a tiling of the general order
        o = options(24, 16, 70, split, abi.RT_METHOD_MIS)
        o.tile_width, o.tile_height = tw, th
        frames[(split, tw, th)] = g.render(cam, o)
        info = g.last_launch_info()
        tiles = ((24 + tw - 1) // tw) * ((16 + th - 1) // th)
        assert info["whole_claims"] == 0 and info["n_items"] == tiles * tw * th * split, info
    g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, 0)
    for (split, tw, th), (img, rays) in frames.items():
        o = options(24, 16, 70, split, abi.RT_METHOD_MIS)
        o.tile_width, o.tile_height = tw, th
        base, base_rays = g.render(cam, o)
        assert img.tobytes() == base.tobytes() and rays == base_rays
