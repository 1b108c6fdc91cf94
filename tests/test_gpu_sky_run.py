"""The sky run of the two-sphere kernels (RT_TUNE_SKY_RUN; csrc/rt_sky_tiles.h, rt_render.hip): tiles proven to see only sky are
flagged when they are claimed and their samples folded without a walk.  (a) the device classifies every tile as the CPU twin does,
byte for byte; (b) frames and ray counts do not depend on the switch, over the ways a launch hands work out; (c) rt_launch_info says
where the run applies; (d) with the run on, the frame is the oracle's."""
import numpy as np
import pytest

import scenes
import sky_tiles_cases as cases
from gpu_support import abi, assert_same_bits

pytestmark = pytest.mark.gpu

RENDER_SIZES = ((64, 40), (97, 53))


@pytest.fixture(scope="module")
def loaded(hb):
    return {name: hb.HipScene(cases.scene(name), device=0) for name in cases.CASES}


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_device_flags_equal_the_host_twins(hb, loaded, tmp_path_factory, name):
    for width, height in cases.SIZES:
        want, _ = cases.host_run(hb, tmp_path_factory, name, width, height)
        cam = hb.camera_new(**cases.camera_params(name, width, height))
        got = hb.selftest_sky_tiles(loaded[name], cam, abi.default_render_opts(width, height, 1))
        assert got.tobytes() == want.tobytes(), (name, width, height, int(got.sum()), int(want.sum()))


def test_other_scenes_and_tilings_flag_nothing(hb):
    ls = scenes.load_ssml("overshadowed")
    g = hb.HipScene(ls.scene, device=0)
    assert not hb.selftest_sky_tiles(g, hb.camera_new(**ls.camera_params), abi.default_render_opts(64, 40, 1)).any()
    pair = hb.HipScene(cases.scene("behind"), device=0)
    opts = abi.default_render_opts(64, 40, 1)
    opts.tile_width, opts.tile_height = 4, 4
    assert not hb.selftest_sky_tiles(pair, hb.camera_new(**cases.camera_params("behind", 64, 40)), opts).any()


def _variants(opts):
    """the launch as it is, as shard 1 of 3 in the packed layout, with the scene read from global memory, from a 64-bit first pass"""
    yield "plain", opts, 1
    o = abi.RenderOpts.from_buffer_copy(opts)
    o.shard_index, o.shard_count, o.output_layout = 1, 3, abi.RT_LAYOUT_SHARD
    yield "shard 1 of 3", o, 1
    yield "scene in global memory", opts, 0
    o = abi.RenderOpts.from_buffer_copy(opts)
    o.sample_begin = (1 << 40) + 12345
    yield "64-bit sample_begin", o, 1


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_frames_do_not_depend_on_the_switch(hb, loaded, name):
    g = loaded[name]
    ran = 0
    for width, height in RENDER_SIZES:
        cam = hb.camera_new(**cases.camera_params(name, width, height))
        for method in (abi.RT_METHOD_MIS, abi.RT_METHOD_NAIVE):
            for spp in (37, 64):
                for split in (1, 4, 0):
                    for share in (0, 16):
                        base = abi.default_render_opts(width, height, spp, method=method, seed=23)
                        base.sample_split = split
                        g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, share)
                        for what, opts, in_lds in _variants(base):
                            label = f"{name} {width}x{height} method={method} spp={spp} split={split} share={share} {what}"
                            g.set_tuning(abi.RT_TUNE_SCENE_IN_LDS, in_lds)
                            g.set_tuning(abi.RT_TUNE_SKY_RUN, 0)
                            off, rays_off = g.render(cam, opts)
                            assert g.last_launch_info()["sky_run"] == 0, label
                            g.set_tuning(abi.RT_TUNE_SKY_RUN, 1)
                            on, rays_on = g.render(cam, opts)
                            info = g.last_launch_info()
                            assert info["sky_run"] == 1 and info["feature_set"] == 3, (label, info)
                            assert_same_bits(on, off, label, nan_equal=True)
                            assert rays_on == rays_off, (label, rays_on, rays_off)
                            ran += 1
    g.set_tuning(abi.RT_TUNE_SCENE_IN_LDS, 1)
    g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, -1)
    g.set_tuning(abi.RT_TUNE_SKY_RUN, -1)
    assert ran == 2 * 2 * 2 * 3 * 2 * 4


def test_launch_info_says_where_the_run_applies(hb, loaded):
    opts = abi.default_render_opts(64, 40, 4, method=abi.RT_METHOD_MIS, seed=1)
    for name in ("rtweekend1", "behind"):
        loaded[name].render(hb.camera_new(**cases.camera_params(name, 64, 40)), opts)  # the default: automatic = on
        assert loaded[name].last_launch_info()["sky_run"] == 1, name
    ls = scenes.load_ssml("overshadowed")
    g = hb.HipScene(ls.scene, device=0)
    g.render(hb.camera_new(**ls.camera_params), opts)
    assert g.last_launch_info()["sky_run"] == 0
    general = hb.HipScene(cases.scene("rtweekend1"), device=0)
    general.set_tuning(abi.RT_TUNE_FEATURE_SET, 0)
    general.render(hb.camera_new(**cases.camera_params("rtweekend1", 64, 40)), opts)
    info = general.last_launch_info()
    assert info["sky_run"] == 0 and info["feature_set"] == 0, info
    with pytest.raises(hb.RtHipError):
        general.set_tuning(abi.RT_TUNE_SKY_RUN, 2)


@pytest.mark.parametrize("method", [abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS])
def test_render_with_the_run_matches_the_oracle(hb, O, method):
    ls = scenes.load_ssml("rtweekend1")
    g, c = hb.HipScene(ls.scene, device=0), O.Scene(ls.scene)
    g.set_tuning(abi.RT_TUNE_SKY_RUN, 1)
    opts = abi.default_render_opts(64, 40, 32, method=method, seed=77)
    img, rays = g.render(hb.camera_new(**ls.camera_params), opts)
    assert g.last_launch_info()["sky_run"] == 1
    ref, ref_rays = c.render(O.camera_new(**ls.camera_params), opts)
    assert np.isfinite(img).all()
    assert np.abs(img.astype(np.float64) - ref.astype(np.float64)).max() < 1e-4
    assert np.array_equal(img, ref), "within 1e-4 but not bit-identical"
    assert rays == ref_rays
