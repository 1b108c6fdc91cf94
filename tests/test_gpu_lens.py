"""rt_render_lens on the GPU (csrc/rt_lens.hip), bit for bit: against the checker (tests/lens_checker.py: the header's ray
arithmetic in numpy f32, the oracle's fixed-ray integrator for every sample) and, with no oracle, against rt_radiance fed the
checker's rays.  test_lens.py shows on the CPU that the frames compared here differ where they should.  Where a sample's value may
be NaN (the MIS prologue returns ahead of the integrators' filter) any NaN equals any NaN; every other word compares as bits."""
import numpy as np
import pytest

import hard_tree_cases
import lens_cases as LN
import lens_checker as LC
import scenes
import sky_cases
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
W, H = LN.W, LN.H
TILES = ((W + 7) // 8) * ((H + 7) // 8)
NAIVE, MIS = abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS
CAMERAS = [(p, 0.0) for p in LN.PROJECTIONS] + [("perspective", LN.APERTURE)]  # the four projections, and the thin lens


def _gpu(hb, name):
    return hb.HipScene(LN.built(name)[0], device=0)


@pytest.mark.parametrize("name", sorted(LN.SCENES))
@pytest.mark.parametrize("method", LN.METHODS)
@pytest.mark.parametrize("projection,aperture", CAMERAS)
def test_frames_are_the_checkers(hb, name, method, projection, aperture):
    """(spp, S) = (4, 1), (4, 2), (7, 3) from sample_begin 5, host entry: the frame, rays_shot, and with a chunk buffer the chunk sums"""
    gpu, cam = _gpu(hb, name), LN.camera(hb, name, projection, aperture)
    for spp, split in LN.FOLDS:
        ref, ref_sums, _ = LN.reference(name, method, projection, spp, split, aperture)
        what = f"{name} method {method} {projection} aperture {aperture} spp {spp} S {split}"
        frame, rays, sums = gpu.render_lens(cam, LN.opts(method, spp, split), chunk_sums=True)
        assert_same_bits(frame, ref, what, nan_equal=True)
        assert rays == LN.rays_shot(name, method, projection, spp, aperture), what  # the oracle integrator's count, sample by sample
        if split > 1:
            assert_same_bits(sums, LC.tiled(ref_sums, W, H), what + ": chunk sums", nan_equal=True)
        else:
            assert sums is None


def _device_run(torch, gpu, cam, o, split, with_sums, off, rays=True, stream=0, bufs=None):
    spec = {"frame": ((H, W, 3), np.float32), "rays": ((2,), np.uint32), "sums": ((max(split, 1), TILES, 8, 8, 3), np.float32)}
    if bufs is None:
        bufs = GuardedBuffers(torch, spec, off=off)
    gpu.render_lens_device(cam, o, bufs.ptr("frame"), bufs.ptr("sums") if with_sums else None,
                           bufs.ptr("rays") if rays and off % 2 == 0 else None, stream=stream)
    torch.cuda.synchronize()
    r = bufs.read("rays")
    return bufs, bufs.read("frame"), (bufs.read("sums") if with_sums else None), int(r[0]) | (int(r[1]) << 32)


@pytest.mark.parametrize("method", LN.METHODS)
def test_device_entry_chunk_sums_and_guards(hb, method):
    """device entry == host entry == checker; the frame is the same with and without the chunk buffer; guard words around both
    buffers, off alignment; the padding lanes of the edge tiles hold +0"""
    import torch
    name = "all_materials"
    gpu, cam = _gpu(hb, name), LN.camera(hb, name, "fisheye")
    for spp, split in ((4, 2), (7, 3)):
        o = LN.opts(method, spp, split)
        ref, ref_sums, _ = LN.reference(name, method, "fisheye", spp, split)
        host, host_rays, host_sums = gpu.render_lens(cam, o, chunk_sums=True)
        got = {}
        for with_sums, off in ((True, 3), (False, 1), (True, 2), (False, 0)):
            bufs, frame, sums, rays = _device_run(torch, gpu, cam, o, split, with_sums, off)
            assert_same_bits(frame, ref, f"device S {split} sums {with_sums} off {off}", nan_equal=True)
            assert frame.tobytes() == host.tobytes()
            if with_sums:
                assert sums.tobytes() == host_sums.tobytes()
                assert_same_bits(sums, LC.tiled(ref_sums, W, H), "chunk sums", nan_equal=True)
                pad = np.ones((8 * 2, 8 * 3), bool)
                pad[:H, :W] = False
                tiled_pad = pad.reshape(2, 8, 3, 8).transpose(0, 2, 1, 3).reshape(TILES, 8, 8)
                assert (sums[:, tiled_pad].view(np.uint32) == 0).all()
            else:
                assert bufs.untouched("sums")
            if off % 2 == 0:
                assert rays == host_rays
            else:
                assert bufs.untouched("rays")
            got[with_sums] = frame
        assert got[True].tobytes() == got[False].tobytes()


def _radiance_fold(gpu, cam, w, h, method, spp, split, seed, begin):
    """the frame from rt_radiance: every pass's rays from the checker, streams = pixel, one sample at sample_begin = the pass; folded
    in numpy.  Returns (frame, inside samples)."""
    passes = np.zeros((spp, w * h, 3), F32)
    streams = np.arange(w * h, dtype=np.uint64)
    inside_count = 0
    for k in range(spp):
        o, d, inside = LC.rays(cam, w, h, seed, begin + k)
        idx = np.flatnonzero(inside)
        passes[k, idx] = gpu.radiance(o[idx], d[idx], streams=streams[idx], method=method, samples=1, seed=seed, sample_begin=begin + k)
        inside_count += len(idx)
    return LC.fold(passes.reshape(spp, h, w, 3), split)[0], inside_count


@pytest.mark.parametrize("projection,aperture,split", [("fisheye", 0.0, 2), ("perspective", LN.APERTURE, 1), ("equirect", 0.0, 3), ("orthographic", 0.0, 2)])
def test_the_chain_tree_against_radiance_queries(hb, projection, aperture, split):
    """64 x 36 x 8, MIS, on the tree whose stacks need more than 64 KB of LDS (the fold record lies behind them): GPU against GPU"""
    sc, cam_params, _, _ = hard_tree_cases.built("chain")
    gpu = hb.HipScene(sc, device=0)
    cam = hb.lens_camera_new(**dict(cam_params, aperture=aperture), projection=projection)
    w, h, spp = 64, 36, 8
    ref, inside = _radiance_fold(gpu, cam, w, h, MIS, spp, split, LN.SEED, LN.BEGIN)
    assert np.unique(ref.reshape(-1, 3), axis=0).shape[0] > 100  # a frame, not a constant
    for with_sums in (False, True):
        frame, _, _ = gpu.render_lens(cam, LN.opts(MIS, spp, split, w, h), chunk_sums=with_sums)
        assert_same_bits(frame, ref, f"chain {projection} S {split} sums {with_sums}", nan_equal=True)
    if projection == "fisheye":
        assert 0.5 * w * h * spp < inside < 0.95 * w * h * spp


@pytest.mark.parametrize("method", LN.METHODS)
def test_a_sky_over_the_lds_limit_against_radiance_queries(hb, method):
    """sky_cases `big_guided` (127 940 bytes of tables: they stay in global memory) over the floor, a panorama: GPU against GPU"""
    sc, cam_params = sky_cases.RENDER_SCENES["floor"]()
    gpu = hb.HipScene(sky_cases.with_sky(sc, "big_guided"), device=0)
    cam = hb.lens_camera_new(**cam_params, projection="equirect")
    w, h, spp = 64, 36, 8
    ref, _ = _radiance_fold(gpu, cam, w, h, method, spp, 2, LN.SEED, LN.BEGIN)
    frame, _, _ = gpu.render_lens(cam, LN.opts(method, spp, 2, w, h))
    assert_same_bits(frame, ref, f"big sky method {method}", nan_equal=True)


@pytest.mark.parametrize("method", LN.METHODS)
def test_schedules_change_no_byte(hb, method):
    """both traversal modes, both walks, a workgroup cap of one (312 pixels on 256 lanes: every lane refills) and none: the bytes and
    the ray count of the first"""
    name = "all_materials"
    cam = LN.camera(hb, name, "fisheye")
    first = None
    for traversal in (0, 1):
        for walk in (0, 1):
            for groups in (1, 0):
                gpu = _gpu(hb, name)
                gpu.set_traversal(traversal)
                gpu.set_tuning(abi.RT_TUNE_WALK, walk)
                gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, groups)
                for with_sums in (False, True):
                    frame, rays, _ = gpu.render_lens(cam, LN.opts(method, 7, 3), chunk_sums=with_sums)
                    if first is None:
                        first = frame.tobytes(), rays
                        assert_same_bits(frame, LN.reference(name, method, "fisheye", 7, 3)[0], "the first schedule", nan_equal=True)
                    assert (frame.tobytes(), rays) == first, (traversal, walk, groups, with_sums)


def test_ray_counters_on_a_view_of_the_sky(hb):
    """only sky: a naive sample is one ray, a MIS sample ends in the prologue ahead of sample_lights (none); a black fisheye sample
    shoots none.  rays_shot is written, not added to."""
    gpu = _gpu(hb, "rtweekend1")
    for projection in LN.SKY_ONLY_PROJECTIONS:
        cam = LN.camera(hb, "rtweekend1", projection, params=LN.SKY_ONLY_CAMERA)
        for spp, split in LN.FOLDS:
            _, _, inside = LN.reference("rtweekend1", NAIVE, projection, spp, split, sky_only=True)
            if projection == "fisheye":
                assert 0.5 * W * H * spp < inside < 0.95 * W * H * spp
            else:
                assert inside == W * H * spp
            for with_sums in (False, True):
                for _ in range(2):  # (twice: written, not added)
                    frame, rays, _ = gpu.render_lens(cam, LN.opts(NAIVE, spp, split), chunk_sums=with_sums)
                    assert rays == inside, (projection, spp, split, with_sums)
                assert_same_bits(frame, LN.reference("rtweekend1", NAIVE, projection, spp, split, sky_only=True)[0], projection, nan_equal=True)
                assert gpu.render_lens(cam, LN.opts(MIS, spp, split), chunk_sums=with_sums)[1] == 0


def test_the_automatic_split_is_the_scenes_rule(hb):
    gpu, cam = _gpu(hb, "all_materials"), LN.camera(hb, "all_materials", "equirect")
    for spp in (4, 64):
        o = LN.opts(MIS, spp, 0)
        split = gpu.auto_sample_split(o)
        auto, auto_rays, sums = gpu.render_lens(cam, o, chunk_sums=True)
        explicit, rays, explicit_sums = gpu.render_lens(cam, LN.opts(MIS, spp, split), chunk_sums=True)
        assert auto.tobytes() == explicit.tobytes() and auto_rays == rays
        assert (sums is None) == (split == 1) and (sums is None or sums.tobytes() == explicit_sums.tobytes())
    assert gpu.auto_sample_split(LN.opts(MIS, 64, 0)) > 1  # (24 x 13 pixels are far fewer than the lanes of the device)


def test_graph_capture_as_a_fresh_scenes_first_call_and_two_streams(hb):
    import torch
    name = "all_materials"
    o = LN.opts(MIS, 4, 2)
    fish, lens = LN.camera(hb, name, "fisheye"), LN.camera(hb, name, "perspective", LN.APERTURE)
    ref_fish, ref_lens = (LN.reference(name, MIS, p, 4, 2, a)[0] for p, a in (("fisheye", 0.0), ("perspective", LN.APERTURE)))
    gpu = _gpu(hb, name)  # fresh: nothing has run on it
    spec = {"frame": ((H, W, 3), np.float32), "sums": ((2, TILES, 8, 8, 3), np.float32)}
    a, b = GuardedBuffers(torch, spec), GuardedBuffers(torch, spec)
    g = capture(torch, lambda s: gpu.render_lens_device(fish, o, a.ptr("frame"), a.ptr("sums"), stream=s))
    assert a.untouched("frame") and a.untouched("sums")
    for _ in range(2):
        a.refill()
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(a.read("frame"), ref_fish, "replay", nan_equal=True)
    # two launches in flight on two streams, two frames
    a.refill()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.render_lens_device(fish, o, a.ptr("frame"), a.ptr("sums"), stream=s1.cuda_stream)
    gpu.render_lens_device(lens, o, b.ptr("frame"), None, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert_same_bits(a.read("frame"), ref_fish, "stream one", nan_equal=True)
    assert_same_bits(b.read("frame"), ref_lens, "stream two", nan_equal=True)
    assert b.untouched("sums")


def test_render_before_and_after_returns_its_own_bytes(hb):
    ls = scenes.load_ssml("rtweekend1")
    gpu, cam = hb.HipScene(ls.scene, device=0), hb.camera_new(**ls.camera_params)
    lens = hb.lens_camera_new(**dict(ls.camera_params, aperture=0.1), projection="perspective")

    def between(opts, image):
        gpu.render_lens(lens, LN.opts(MIS, 4, 2), chunk_sums=True)
    assert_render_unaffected(gpu, cam, between)
    # the same rays in distribution, other draws: NOT rt_render's bytes even at lens radius 0
    o = LN.opts(MIS, 4, 1)
    assert gpu.render_lens(hb.lens_camera_new(**ls.camera_params), o)[0].tobytes() != gpu.render(cam, o)[0].tobytes()


def test_a_multi_device_scene_is_refused(hb):
    gpu = hb.HipScene(LN.built("rtweekend1")[0], devices=[0, 0])
    with pytest.raises(hb.RtHipError) as e:
        gpu.render_lens(LN.camera(hb, "rtweekend1", "perspective"), LN.opts(MIS, 4, 1))
    assert e.value.code == abi.RT_ERR_UNSUPPORTED
