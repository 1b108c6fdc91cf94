"""rt_render_lens_aov and rt_render_lens_denoised on the GPU (csrc/rt_aov_lens.hip), bit for bit: every channel against the checker
(tests/lens_aov_checker.py: lens_checker's rays, aov_chain_checker's chains over the oracle's check_hit), the edge shapes, the
identities the header states, the deep trees, graph capture, two streams, no side effect, and the one-call denoised frame against
the same steps composed from the public entry points.  test_lens_aov.py shows on the CPU that the frames compared here differ where
they should and hold no NaN, so floats compare as words -- except on the trees of hard_tree_cases, whose geometry is non-finite on
purpose (there any NaN equals any NaN, as in test_gpu_hard_trees.py)."""
import numpy as np
import pytest

import denoise_checker as DK
import hard_tree_cases as HT
import lens_aov_cases as LA
import lens_aov_checker as LK
import scenes
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
W, H = LA.W, LA.H
CHANNELS = LK.CHANNELS
SPEC = {c: ((H, W, 3) if c in ("albedo", "normal") else (H, W), np.uint32 if c in ("primitive", "material") else np.float32) for c in CHANNELS}


def _gpu(hb, name):
    return hb.HipScene(LA.built(name)[0], device=0)


def _chain(max_chain):
    """the keyword of the binding: max_chain 0 goes as NULL options in every other call, so both forms are compared everywhere"""
    return {"max_chain": max_chain}


def assert_channels(got, ref, what, nan_equal=False):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for c in ref:
        assert_same_bits(got[c], ref[c], f"{what} {c}", nan_equal=nan_equal)


def _modes(gpu):
    """forced exhaustive / pruned (both walks) / automatic: the same bytes"""
    for mode in (0, 1, -1):
        gpu.set_traversal(mode)
        for walk in ((0, 1) if mode == 1 else (0,)):
            gpu.set_tuning(abi.RT_TUNE_WALK, walk)
            yield mode, walk


@pytest.mark.parametrize("name", sorted(LA.SCENES))
@pytest.mark.parametrize("projection,aperture", LA.CAMERAS)
def test_channels_are_the_checkers(hb, name, projection, aperture):
    """3 passes from sample_begin 5, first hit and max_chain 8, every traversal mode and walk, the host entry"""
    gpu, cam = _gpu(hb, name), LA.camera(hb, name, projection, aperture)
    for chain in LA.CHAINS:
        ref, _ = LA.reference(name, projection, aperture, chain)
        for mode, walk in _modes(gpu):
            got = gpu.render_lens_aov(cam, LA.opts(), **(_chain(chain) if chain or mode == 0 else {}))
            assert_channels(got, ref, f"{name} {projection} aperture {aperture} max_chain {chain} traversal {mode} walk {walk}")


@pytest.mark.parametrize("w,h", [(2, 2), (9, 8), (16, 8)])
def test_edge_frames(hb, w, h):
    """2 x 2: 60 padding lanes; 9 x 8: a tile of one column; 16 x 8: no padding lane"""
    name = LA.MIRRORS
    gpu = _gpu(hb, name)
    for projection, aperture in (("perspective", LA.LN.APERTURE), ("fisheye", 0.0), ("equirect", 0.0)):
        ref, _ = LA.reference(name, projection, aperture, 8, w=w, h=h)
        got = gpu.render_lens_aov(LA.camera(hb, name, projection, aperture), LA.opts(w=w, h=h), max_chain=8)
        assert_channels(got, ref, f"{w}x{h} {projection}")


@pytest.mark.parametrize("seed,begin", [((1 << 32) + 3, (1 << 32) - 2), (0xFFFFFFFF00000005, (1 << 63) + 1), (7, (1 << 64) - 2)])
def test_64_bit_streams(hb, seed, begin):
    """seed and sample_begin as 64-bit values: the carry of sample_begin + k into the high word, both high words set, and the sum
    wrapping past 2^64"""
    name = "all_materials"
    gpu, cam = _gpu(hb, name), LA.camera(hb, name, "perspective", LA.LN.APERTURE)
    ref, _ = LA.reference(name, "perspective", LA.LN.APERTURE, 8, spp=4, seed=seed, begin=begin)
    got = gpu.render_lens_aov(cam, LA.opts(spp=4, seed=seed, begin=begin), max_chain=8)
    assert_channels(got, ref, f"seed {seed:#x} begin {begin:#x}")
    low, _ = LA.reference(name, "perspective", LA.LN.APERTURE, 8, spp=4, seed=seed & 0xFFFFFFFF, begin=begin & 0xFFFFFFFF)
    assert low["depth"].tobytes() != ref["depth"].tobytes()  # the high words reach the stream


@pytest.mark.parametrize("w,h", [(24, 8), (8, 24)])
def test_a_220_degree_fisheye_with_lanes_that_never_walk(hb, w, h):
    """whole rows (8 x 24) and a whole column (24 x 8) of pixels whose every sample is black: lanes that leave the loop without a
    walk, next to lanes of the same wave that walk chains"""
    name = "all_materials"
    gpu, cam = _gpu(hb, name), LA.camera(hb, name, "fisheye", fov=LA.FISHEYE_220)
    for chain in LA.CHAINS:
        ref, inside = LA.reference(name, "fisheye", max_chain=chain, w=w, h=h, fov=LA.FISHEYE_220)
        assert (~inside.any(axis=0)).all(axis=0 if w == 24 else 1).any()
        for mode, walk in _modes(gpu):
            got = gpu.render_lens_aov(cam, LA.opts(w=w, h=h), max_chain=chain)
            assert_channels(got, ref, f"{w}x{h} max_chain {chain} traversal {mode} walk {walk}")


def test_a_lens_of_radius_4_with_origins_inside_the_ground_sphere(hb):
    gpu, cam = _gpu(hb, LA.MIRRORS), LA.camera(hb, LA.MIRRORS, "perspective", 8.0)
    for chain in LA.CHAINS:
        ref, _ = LA.reference(LA.MIRRORS, "perspective", 8.0, chain)
        assert_channels(gpu.render_lens_aov(cam, LA.opts(), max_chain=chain), ref, f"lens radius 4 max_chain {chain}")


def test_identities(hb):
    """NULL options are max_chain 0; any max_chain on a scene without followed materials gives the NULL-options bytes; a perspective
    camera at lens radius 0 does not give rt_render_aov's bytes"""
    for name, equal in ((LA.MIRRORS, False), ("rtweekend1", True)):
        assert bool(LA.followed_materials(name)) != equal
        gpu = _gpu(hb, name)
        for projection, aperture in LA.CAMERAS:
            cam = LA.camera(hb, name, projection, aperture)
            null = gpu.render_lens_aov(cam, LA.opts())
            zero = gpu.render_lens_aov(cam, LA.opts(), max_chain=0, fuzz_limit=0.5)
            deep = gpu.render_lens_aov(cam, LA.opts(), max_chain=64)
            for c in CHANNELS:
                assert null[c].tobytes() == zero[c].tobytes(), (name, projection, c)
            assert all(null[c].tobytes() == deep[c].tobytes() for c in CHANNELS) == equal, (name, projection)
    name = "all_materials"
    gpu = _gpu(hb, name)
    pinhole = gpu.render_aov(hb.camera_new(**LA.built(name)[1]), LA.opts())
    lens = gpu.render_lens_aov(LA.camera(hb, name, "perspective"), LA.opts())
    assert pinhole["normal"].tobytes() != lens["normal"].tobytes()
    assert np.abs(pinhole["coverage"] - lens["coverage"]).mean() < 0.1  # the same image all the same


def _device_run(torch, gpu, cam, o, channels, off=0, stream=0, bufs=None, **chain):
    if bufs is None:
        bufs = GuardedBuffers(torch, SPEC, off=off)
    gpu.render_lens_aov_device(cam, o, bufs.ptrs(channels), stream=stream, **chain)
    torch.cuda.synchronize()
    return bufs


def test_device_entry_and_a_null_channel_is_not_written(hb):
    """the device entry into guarded buffers off alignment: the bytes of the host entry and of the checker; a channel left out
    keeps its sentinel, and the others do not change"""
    import torch
    name = LA.MIRRORS
    gpu, cam = _gpu(hb, name), LA.camera(hb, name, "fisheye")
    ref, _ = LA.reference(name, "fisheye", 0.0, 8)
    host = gpu.render_lens_aov(cam, LA.opts(), max_chain=8)
    subsets = [CHANNELS, ("bounces",), ("depth",), ("albedo", "primitive"), ("normal", "coverage", "material"), tuple(c for c in CHANNELS if c != "albedo")]
    for off, channels in enumerate(subsets):
        bufs = _device_run(torch, gpu, cam, LA.opts(), channels, off=off % 4, max_chain=8)
        for c in CHANNELS:
            if c in channels:
                got = bufs.read(c)
                assert_same_bits(got, ref[c], f"device {channels} {c}", nan_equal=False)
                assert got.tobytes() == host[c].tobytes()
            else:
                assert bufs.untouched(c), (channels, c)
    with pytest.raises(hb.RtHipError) as e:
        gpu.render_lens_aov_device(cam, LA.opts(), {})
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", list(HT.CASES))
def test_hard_trees(hb, name):
    """the equidistant fisheye of the case's own camera, 40 x 27 x 2, max_chain 8, on the trees built to break walks; the last one
    keeps its four waves' stacks in more than 64 KB of LDS"""
    sc, cam_params, cpu, _ = HT.built(name)
    gpu = hb.HipScene(sc, device=0)
    cam = hb.lens_camera_new(**cam_params, projection="fisheye")
    flat, inside = LK.aovs(sc, cpu, cam, HT.W, HT.H, HT.SPP, seed=HT.SEED, max_chain=8, return_inside=True)
    ref = LK.framed(flat, HT.W, HT.H)
    assert inside.any() and not inside.all()
    o = abi.default_render_opts(HT.W, HT.H, HT.SPP, seed=HT.SEED)
    for mode, walk in _modes(gpu):
        assert_channels(gpu.render_lens_aov(cam, o, max_chain=8), ref, f"{name} traversal {mode} walk {walk}", nan_equal=True)


def test_graph_capture_as_a_fresh_scenes_first_call_and_two_streams(hb):
    import torch
    name = LA.MIRRORS
    fish, lens = LA.camera(hb, name, "fisheye"), LA.camera(hb, name, "perspective", LA.LN.APERTURE)
    ref_fish, ref_lens = LA.reference(name, "fisheye", 0.0, 8)[0], LA.reference(name, "perspective", LA.LN.APERTURE, 0)[0]
    gpu = _gpu(hb, name)  # fresh: nothing has run on it
    a, b = GuardedBuffers(torch, SPEC), GuardedBuffers(torch, SPEC)
    g = capture(torch, lambda s: gpu.render_lens_aov_device(fish, LA.opts(), a.ptrs(), stream=s, max_chain=8))
    assert all(a.untouched(c) for c in CHANNELS)
    for _ in range(2):
        a.refill()
        g.replay()
        torch.cuda.synchronize()
        assert_channels(a.read_all(), ref_fish, "replay")
    # two launches in flight on two streams, two cameras
    a.refill()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.render_lens_aov_device(fish, LA.opts(), a.ptrs(), stream=s1.cuda_stream, max_chain=8)
    gpu.render_lens_aov_device(lens, LA.opts(), b.ptrs(), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert_channels(a.read_all(), ref_fish, "stream one")
    assert_channels(b.read_all(), ref_lens, "stream two")


def test_render_before_and_after_returns_its_own_bytes(hb):
    ls = scenes.load_ssml("rtweekend1")
    gpu, cam = hb.HipScene(ls.scene, device=0), hb.camera_new(**ls.camera_params)
    lens = hb.lens_camera_new(**dict(ls.camera_params, aperture=0.1), projection="perspective")

    def between(opts, image):
        gpu.render_lens_aov(lens, LA.opts(), max_chain=8)
    assert_render_unaffected(gpu, cam, between)


def test_a_multi_device_scene_is_refused(hb):
    gpu = hb.HipScene(LA.built("rtweekend1")[0], devices=[0, 0])
    cam = LA.camera(hb, "rtweekend1", "perspective")
    for call in (lambda: gpu.render_lens_aov(cam, LA.opts()), lambda: gpu.render_lens_denoised(cam, LA.opts(spp=4))):
        with pytest.raises(hb.RtHipError) as e:
            call()
        assert e.value.code == abi.RT_ERR_UNSUPPORTED


@pytest.mark.parametrize("projection,aperture", [("perspective", LA.LN.APERTURE), ("fisheye", 0.0)])
@pytest.mark.parametrize("split", [1, 2])
def test_render_lens_denoised_is_its_parts(hb, projection, aperture, split):
    """24 x 13, S = 4: two rt_render_lens halves, rt_render_lens_aov of all passes, the combine in numpy as denoise_checker states it,
    rt_denoise -- bit for bit; with and without the noisy frame; rays_shot the sum of the halves"""
    name = LA.MIRRORS
    gpu, cam = _gpu(hb, name), LA.camera(hb, name, projection, aperture)
    spp, method = 4, abi.RT_METHOD_MIS
    o = LA.LN.opts(method, spp, split)
    for chain in ({}, {"max_chain": 8}):
        clean, noisy, rays = gpu.render_lens_denoised(cam, o, **chain)
        halves, half_rays = [], 0
        for begin in (LA.BEGIN, LA.BEGIN + spp // 2):
            img, r, _ = gpu.render_lens(cam, LA.LN.opts(method, spp // 2, split, begin=begin))
            halves.append(img)
            half_rays += r
        assert_same_bits(noisy, (halves[0] + halves[1]) * F32(0.5), f"{projection} noisy", nan_equal=True)
        assert rays == half_rays
        aov = gpu.render_lens_aov(cam, o, channels=("albedo", "normal", "depth"), **chain)
        var = DK.halves_variance(halves[0], halves[1], aov["albedo"])
        assert_same_bits(clean, gpu.denoise(noisy, aov, variance=var), f"{projection} {chain} clean", nan_equal=True)
        only_clean, none, rays_again = gpu.render_lens_denoised(cam, o, noisy=False, **chain)
        assert none is None and rays_again == rays and only_clean.tobytes() == clean.tobytes()
        assert (clean != noisy).any()  # the filter does something
    # a non-default filter option reaches the filter
    clean3, _, _ = gpu.render_lens_denoised(cam, o, hb.denoise_opts(0, 0, iterations=3), max_chain=8)
    assert_same_bits(clean3, gpu.denoise(noisy, aov, variance=var, iterations=3), "iterations 3", nan_equal=True)
