"""The host's side of whole-pixel claims (rt_api.cpp plan_work_items, reached through rt_plan_work_items -- the function
plan_render_launch itself calls, so what rt_launch_info reports after a render: tests/test_gpu_whole_pixel_claims.py compares
the two on the device): how many of a launch's claims are whole tiles and how many work items the launch has, for a table of
(tiles, split, share, shard count).  No GPU."""
import pytest

import scenes

abi = scenes.abi


def restated(width, height, tile_w, tile_h, split, share, shard_index, shard_count, resident_waves=0):
    """a dozen lines of Python for what the planner must return"""
    tiles_x, tiles_y = -(-width // tile_w), -(-height // tile_h)
    n_tiles = tiles_x * tiles_y
    tiles = (n_tiles - shard_index + shard_count - 1) // shard_count if n_tiles > shard_index else 0
    tiled = (tile_w * tile_h == 64 and tile_w & (tile_w - 1) == 0 and width < 65536 and height < 65536
             and split & (split - 1) == 0 and split <= 64)
    if not tiled or split == 1:
        return 0, tiles * tile_w * tile_h * split
    whole = tiles * share // 16
    if share == -1:  # the library's own choice: half the tiles, at most 3 per resident wave, at least 2.5 per resident wave left
        whole = min(tiles // 2, max(0, tiles - (5 * resident_waves + 1) // 2), 3 * resident_waves)
    return whole, 64 * (whole + (tiles - whole) * split)


FRAMES = [(24, 16), (19, 13), (8, 8), (1920, 1080), (65536, 8)]  # 6, 6, 1, 32 400 and 8 192 tiles; the last too wide for the tiled order
TILINGS = [(8, 8), (16, 4), (64, 1), (4, 4), (5, 3)]
SPLITS = [1, 2, 4, 5, 16, 64]
SHARES = [0, 1, 8, 10, 15, 16]


@pytest.mark.parametrize("shard_count", [1, 2, 3, 4, 7])
def test_whole_claims_and_work_items(hb, shard_count):
    checked = 0
    for (w, h) in FRAMES:
        for (tw, th) in TILINGS:
            for split in SPLITS:
                for share in SHARES:
                    for idx in range(shard_count):  # (8 x 8 at seven shards: six of them own no tile at all)
                        o = abi.default_render_opts(w, h, 64, seed=1)
                        o.tile_width, o.tile_height, o.shard_index, o.shard_count = tw, th, idx, shard_count
                        want = restated(w, h, tw, th, split, share, idx, shard_count)
                        assert hb.plan_work_items(o, split, share) == want, (w, h, tw, th, split, share, idx, shard_count)
                        checked += 1
    assert checked == len(FRAMES) * len(TILINGS) * len(SPLITS) * len(SHARES) * shard_count


def test_the_automatic_share_goes_by_tiles_per_resident_wave(hb):
    """6 144 resident waves is what an MI355X holds of the pair kernel (256 CUs x 2 workgroups x 12 waves).  The frames: the headline
    1080p (5.27 tiles per wave: half the tiles), a device's eighth of it and 640 x 360 (0.66 and 0.59: none), 2560 x 1440 (9.4:
    capped at three whole tiles per wave), and frames around the 2.5 tiles per wave below which nothing is handed out whole"""
    waves = 6144
    def plan(w, h, shards=1, idx=0, split=16, r=waves):
        o = abi.default_render_opts(w, h, 1024, seed=1)
        o.shard_index, o.shard_count = idx, shards
        got = hb.plan_work_items(o, split, -1, r)
        assert got == restated(w, h, 8, 8, split, -1, idx, shards, r), (w, h, shards, idx, split, r)
        return got[0]
    assert plan(1920, 1080) == 16200                       # 32 400 tiles: half of them, 17 040 would still leave 2.5 per wave
    assert [plan(1920, 1080, 8, i) for i in range(8)] == [0] * 8
    assert plan(640, 360) == 0
    assert plan(2560, 1440) == 3 * waves                   # 57 600 tiles: the cap per wave, not the half
    assert plan(1920, 1080, split=1) == 0
    assert plan(1024, 960) == 0 and plan(1024, 968) == 128 and plan(1024, 1256) == 4736  # 15 360 tiles = 2.5 per wave, 15 488, 20 096
    assert plan(1920, 1080, r=0) == 0 and plan(1920, 1080, r=1) == 3  # no device, a device of one wave
    for r in (1, 7, 100, 6144, 10 ** 6):
        for (w, h) in FRAMES:
            for shards in (1, 3):
                for split in (1, 4, 16):
                    plan(w, h, shards, shards - 1, split, r)


def test_edges_of_the_share(hb):
    o = abi.default_render_opts(24, 16, 64, seed=1)
    assert hb.plan_work_items(o, 16, 0) == (0, 6 * 64 * 16)  # share 0: every tile chunk by chunk, the items of pixels x split
    assert hb.plan_work_items(o, 16, 16) == (6, 6 * 64)      # share 16: whole-pixel claims only, one item per pixel
    assert hb.plan_work_items(o, 16, 8) == (3, 64 * (3 + 3 * 16))
    assert hb.plan_work_items(o, 1, 16) == (0, 6 * 64)       # S = 1 has no chunks to fold
    o.shard_index, o.shard_count = 6, 7                       # a shard without a tile
    assert hb.plan_work_items(o, 16, 8) == (0, 0)
    for bad_split, bad_share in ((0, 8), (16, -2), (16, 17)):
        with pytest.raises(Exception):
            hb.plan_work_items(abi.default_render_opts(24, 16, 64, seed=1), bad_split, bad_share)
