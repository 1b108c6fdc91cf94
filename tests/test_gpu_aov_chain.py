"""Specular-chain AOV buffers (rt_render_aov_chain) on the GPU against the CPU checker (tests/aov_chain_checker.py): every
comparison is bit-exact (NaN == NaN).  Then the quality of rt_denoise / rt_upscale under chain guides next to first-hit guides on
a scene with a perfect mirror and a glass sphere (figures: DESIGN.md section 14)."""
import itertools

import numpy as np
import pytest

import aov_chain_checker as KC
import aov_checker as K
import scenes
from gpu_support import (CAMERA_16_9, QUALITY_CAMERA, QUALITY_GLASS, QUALITY_MIRROR, GuardedBuffers, assert_render_unaffected,
                         assert_same_bits, capture, quality_scene, ssml_scene)

pytestmark = pytest.mark.gpu
abi = scenes.abi
W, H, SPP = 64, 36, 4
F32 = np.float32


def nested_and_facing():
    """delta surfaces behind delta surfaces: a mirror ball inside a glass ball, a glass ball inside a glass ball, two facing
    mirror walls with a textured ball between them, a fuzzy mirror -- over a checkered Lambertian floor"""
    sc = scenes.SceneDescription()
    sc.sphere((0, -1000, 0), 1000.0, sc.lambertian(sc.checkered((0.9, 0.9, 0.9), (0.2, 0.3, 0.6)), 0.8))
    glass = sc.refract(sc.solid((0.95, 1.0, 0.9)), 1.5)
    sc.sphere((-1.3, 0.8, 0.0), 0.8, glass)
    sc.sphere((-1.3, 0.8, 0.0), 0.35, sc.reflect(sc.lerp((0.9, 0.6, 0.3), (0.3, 0.6, 0.9)), 0.0))
    sc.sphere((1.3, 0.8, 0.0), 0.8, sc.refract(sc.solid((1.0, 1.0, 1.0)), 1.3))
    sc.sphere((1.3, 0.8, 0.0), 0.4, sc.refract(sc.checkered((1.0, 0.8, 0.8), (0.8, 0.8, 1.0)), 1.9))
    mirror = sc.reflect(sc.solid((0.9, 0.9, 0.95)), 0.0)
    for x, nx in ((-3.0, 1.0), (3.0, -1.0)):  # two walls facing each other across the scene
        n = (nx, 0.0, 0.0)
        sc.triangle([(x, 0.0, -3.0), (x, 0.0, 3.0), (x, 3.0, 3.0)], [n, n, n], mirror)
        sc.triangle([(x, 0.0, -3.0), (x, 3.0, 3.0), (x, 3.0, -3.0)], [n, n, n], mirror)
    sc.sphere((0.0, 0.5, -1.0), 0.5, sc.lambertian(sc.solid((0.8, 0.3, 0.2)), 0.7))
    sc.sphere((0.0, 0.4, 1.2), 0.4, sc.reflect(sc.solid((0.8, 0.8, 0.8)), 0.25))
    sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (16, 8))
    return sc


NESTED_CAMERA = dict(origin=(0.0, 1.6, 6.5), lookat=(0.0, 0.7, 0.0), vup=(0.0, 1.0, 0.0), fov=50.0, aspect_ratio=CAMERA_16_9,
                     aperture=0.0, focus_dist=10.0)


SCENES = {
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "nested_and_facing": lambda: (nested_and_facing(), NESTED_CAMERA),
    "quality_scene": lambda: (quality_scene(), QUALITY_CAMERA),
}
SCENES.update({f"random_everything_{seed}": (lambda seed=seed: scenes.random_everything(seed)) for seed in range(6)})
CHAINS = [(0, 0.0), (1, 0.0), (2, 0.0), (8, 0.0), (1, 1.0), (8, 1.0)]  # (max_chain, fuzz_limit)


def assert_aovs_equal(gpu, ref, what):
    assert set(gpu) == set(ref), (what, sorted(gpu), sorted(ref))
    for name in ref:
        assert_same_bits(gpu[name], ref[name], f"{what} {name}", nan_equal=True)


def _reference(sc, cpu, cam, w, h, spp, seed, sample_begin, max_chain, fuzz_limit, pixels=None):
    r = KC.aovs(sc, cpu, cam, w, h, spp, seed=seed, sample_begin=sample_begin, pixels=pixels, max_chain=max_chain, fuzz_limit=fuzz_limit)
    if pixels is None:
        r = {k: v.reshape((h, w, 3) if v.ndim == 2 else (h, w)) for k, v in r.items()}
    return r


@pytest.mark.parametrize("name", list(SCENES))
def test_chain_aovs_match_the_checker(hb, O, name):
    sc, cam_params = SCENES[name]()
    gpu, cpu = hb.HipScene(sc, device=0), O.Scene(sc)
    cam_g, cam_c = hb.camera_new(**cam_params), O.camera_new(**cam_params)
    followed_somewhere = False
    for (max_chain, fuzz_limit), sample_begin in zip(CHAINS, (0, 5, 0, 3, 0, 7)):
        opts = abi.default_render_opts(W, H, SPP, seed=3)
        opts.sample_begin = sample_begin
        ref = _reference(sc, cpu, cam_c, W, H, SPP, 3, sample_begin, max_chain, fuzz_limit)
        what = f"{name} max_chain={max_chain} fuzz_limit={fuzz_limit} sample_begin={sample_begin}"
        assert_aovs_equal(gpu.render_aov_chain(cam_g, opts, max_chain=max_chain, fuzz_limit=fuzz_limit), ref, what + " auto traversal")
        for mode in (0, 1):  # forced exhaustive / pruned: the same bytes
            gpu.set_traversal(mode)
            assert_aovs_equal(gpu.render_aov_chain(cam_g, opts, max_chain=max_chain, fuzz_limit=fuzz_limit), ref, what + f" traversal={mode}")
        gpu.set_traversal(-1)
        assert (ref["bounces"] <= max_chain).all()
        followed_somewhere |= bool(ref["bounces"].max() > 0)
    assert followed_somewhere, "the scene shows no followed surface: the case tests nothing"


def test_max_chain_zero_and_scenes_without_delta_surfaces_give_the_first_hit_bytes(hb):
    for name in list(SCENES) + ["rtweekend1", "overshadowed"]:
        if name in SCENES:
            sc, cam_params = SCENES[name]()
        else:
            sc, cam_params = ssml_scene(name)
        gpu = hb.HipScene(sc, device=0)
        cam = hb.camera_new(**cam_params)
        opts = abi.default_render_opts(W, H, 16, seed=6)
        opts.sample_begin = 2
        first = gpu.render_aov(cam, opts)
        chains = [0] if name in SCENES else [0, 8]  # rtweekend1, overshadowed: no Reflect / Refract, any max_chain
        for max_chain in chains:
            got = gpu.render_aov_chain(cam, opts, max_chain=max_chain, fuzz_limit=1.0)
            for ch in abi.AOV_CHANNELS:
                assert_same_bits(got[ch], first[ch], f"{name} max_chain={max_chain} {ch}", nan_equal=True)
            assert (got["bounces"] == 0.0).all()


def test_every_channel_subset_gives_the_same_bytes(hb):
    sc, cam_params = SCENES["nested_and_facing"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(W, H, 3, seed=9)
    full = gpu.render_aov_chain(cam, opts)
    for k in range(1, len(abi.AOV_CHAIN_CHANNELS)):
        for subset in itertools.combinations(abi.AOV_CHAIN_CHANNELS, k):
            got = gpu.render_aov_chain(cam, opts, channels=subset)
            assert set(got) == set(subset)
            for name in subset:
                assert_same_bits(got[name], full[name], f"subset {subset} {name}", nan_equal=True)


@pytest.mark.parametrize("size", [(2, 2), (3, 5), (9, 7), (65, 37)])
def test_ragged_and_tiny_frames(hb, O, size):
    w, h = size
    sc, cam_params = SCENES["nested_and_facing"]()
    gpu, cpu = hb.HipScene(sc, device=0), O.Scene(sc)
    opts = abi.default_render_opts(w, h, 3, seed=12)
    opts.sample_begin = 4
    ref = _reference(sc, cpu, O.camera_new(**cam_params), w, h, 3, 12, 4, 8, 0.0)
    assert_aovs_equal(gpu.render_aov_chain(hb.camera_new(**cam_params), opts), ref, f"{w}x{h}")


def test_tiles_of_a_1080p_frame(hb, O):
    sc, cam_params = SCENES["all_materials"]()
    gpu, cpu = hb.HipScene(sc, device=0), O.Scene(sc)
    w, h, spp = 1920, 1080, 2
    opts = abi.default_render_opts(w, h, spp, seed=1)
    got = gpu.render_aov_chain(hb.camera_new(**cam_params), opts)
    tiles_x, tiles_y = w // 8, h // 8
    rng = np.random.default_rng(0)
    tiles = {(0, 0), (tiles_x - 1, tiles_y - 1), (0, tiles_y - 1), (tiles_x - 1, 0)}
    glass = np.argwhere(got["bounces"] >= 2.0)  # tiles that see through the glass ball, then random ones
    for y, x in glass[:: max(1, len(glass) // 12)]:
        tiles.add((int(x) // 8, int(y) // 8))
    while len(tiles) < 40:
        tiles.add((int(rng.integers(0, tiles_x)), int(rng.integers(0, tiles_y))))
    pixels = K.tile_pixels(w, h, sorted(tiles))
    ref = _reference(sc, cpu, O.camera_new(**cam_params), w, h, spp, 1, 0, 8, 0.0, pixels=pixels)
    flat = {k: v.reshape(w * h, -1) if v.ndim == 3 else v.reshape(w * h) for k, v in got.items()}
    for name in ref:
        assert_same_bits(flat[name][pixels], ref[name], f"1080p tiles {name}", nan_equal=True)
    assert len(glass) > 0 and ref["bounces"].max() >= 2.0
    assert ((got["primitive"] == abi.AOV_NO_ID) == (got["material"] == abi.AOV_NO_ID)).all()


def device_chain(torch, w, h, off=0):
    """device buffers `off` floats past an aligned base, with guard values before and after every channel"""
    return GuardedBuffers(torch, {name: ((h, w, 3) if name in ("albedo", "normal") else (h, w),
                                         np.uint32 if name in ("primitive", "material") else np.float32)
                                  for name in abi.AOV_CHAIN_CHANNELS}, off=off)


def test_device_entry_equals_host_entry_off_alignment_with_guards(hb):
    import torch
    sc, cam_params = SCENES["nested_and_facing"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    w, h = 67, 37
    opts = abi.default_render_opts(w, h, 5, seed=4)
    opts.sample_begin = 3
    ref = gpu.render_aov_chain(cam, opts, max_chain=6, fuzz_limit=0.5)
    for off in (0, 1, 3):
        run = device_chain(torch, w, h, off)
        torch.cuda.synchronize()
        gpu.render_aov_chain_device(cam, opts, run.ptrs(), max_chain=6, fuzz_limit=0.5)
        torch.cuda.synchronize()
        assert_aovs_equal(run.read_all(), ref, f"device entry off={off}")
    run = device_chain(torch, w, h, 1)  # a subset: the other buffers stay untouched
    torch.cuda.synchronize()
    gpu.render_aov_chain_device(cam, opts, run.ptrs(("depth", "bounces")), max_chain=6, fuzz_limit=0.5)
    torch.cuda.synchronize()
    got = run.read_all()
    assert_same_bits(got["depth"], ref["depth"], "subset depth", nan_equal=True)
    assert_same_bits(got["bounces"], ref["bounces"], "subset bounces", nan_equal=True)
    assert (got["material"] == run.guard).all() and (got["albedo"].view(np.uint32) == run.guard).all()


def test_determinism_across_streams(hb):
    import torch
    sc, cam_params = SCENES["random_everything_3"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(W, H, 8, seed=21)
    ref = gpu.render_aov_chain(cam, opts, fuzz_limit=1.0)
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    runs = [device_chain(torch, W, H) for _ in streams]
    torch.cuda.synchronize()
    for _ in range(2):
        for s, run in zip(streams, runs):  # in flight together
            gpu.render_aov_chain_device(cam, opts, run.ptrs(), stream=s.cuda_stream, fuzz_limit=1.0)
    torch.cuda.synchronize()
    for i, run in enumerate(runs):
        assert_aovs_equal(run.read_all(), ref, f"stream {i}")


def test_graph_captured_from_the_first_call_replays_the_eager_bytes(hb):
    """no warm-up: the scene's first chain call of any kind is the captured one"""
    import torch
    sc, cam_params = SCENES["nested_and_facing"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(W, H, 6, seed=17)
    dev = torch.device("cuda", 0)
    run = device_chain(torch, W, H)
    g = capture(torch, lambda stream: gpu.render_aov_chain_device(cam, opts, run.ptrs(), stream=stream))
    assert all(run.untouched(name) for name in run.buf)  # capture ran nothing
    eager = gpu.render_aov_chain(cam, opts)
    for _ in range(2):
        run.refill()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        assert_aovs_equal(run.read_all(), eager, "graph replay")


def test_no_side_effects_on_render(hb):
    sc, cam_params = ssml_scene("overshadowed")
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    assert_render_unaffected(gpu, cam, lambda opts, img: gpu.render_aov_chain(cam, opts))


def test_multi_device_head_scene(hb):
    import torch
    sc, cam_params = SCENES["random_everything_3"]()
    single, multi = hb.HipScene(sc, device=0), hb.HipScene(sc, devices=[0, 0])
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(W, H, 8, seed=6)
    ref = single.render_aov_chain(cam, opts, fuzz_limit=1.0)
    assert_aovs_equal(multi.render_aov_chain(cam, opts, fuzz_limit=1.0), ref, "devices=[0, 0]")
    run = device_chain(torch, W, H)
    torch.cuda.synchronize()
    multi.render_aov_chain_device(cam, opts, run.ptrs(), fuzz_limit=1.0)
    torch.cuda.synchronize()
    assert_aovs_equal(run.read_all(), ref, "devices=[0, 0] device entry")


# ---- quality: the protocol of the denoiser's test (display-space MSE against a 4096-pass render, 320 x 180, 16 MIS passes) ----
def _display_se(img, ref):
    f = lambda a: np.clip(a.astype(np.float64), 0.0, 1.0) ** (1 / 2.2)  # noqa: E731
    return ((f(img) - f(ref)) ** 2).mean(axis=2)


def delta_shares(O, sc, cam_params, w, h):
    """(mirror mask, glass mask) [h, w]: the first hit of the pixel-centre ray, by the oracle's check_hit"""
    cam = O.camera_new(**cam_params)
    pixels = np.arange(w * h)
    x, y = (pixels % w).astype(F32), (pixels // w).astype(F32)
    u, v = (x + F32(0.5)) / F32(w - 1), F32(1.0) - (y + F32(0.5)) / F32(h - 1)
    o, ll, hz, vt = (np.array(a[:], F32) for a in (cam.origin, cam.lower_left, cam.horizontal, cam.vertical))
    d = ((ll[None, :] + hz[None, :] * u[:, None]) + vt[None, :] * v[:, None]) - o[None, :]
    hit = O.Scene(sc).check_hit(np.broadcast_to(o, d.shape).copy(), d.astype(F32))
    found = hit["index"] != np.uint64(abi.NO_INDEX)
    return ((found & (hit["material"] == QUALITY_MIRROR)).reshape(h, w), (found & (hit["material"] == QUALITY_GLASS)).reshape(h, w))


def test_quality_scene_shows_enough_delta_pixels(O):
    mirror, glass = delta_shares(O, quality_scene(), QUALITY_CAMERA, 320, 180)
    assert (mirror | glass).mean() >= 0.05, (mirror.mean(), glass.mean())
    assert mirror.mean() >= 0.02 and glass.mean() >= 0.02


def test_chain_guides_beat_first_hit_guides_on_delta_pixels(hb, O):
    """rt_denoise twice on the SAME colour and variance, once under first-hit guides, once under chain guides; then both through
    rt_upscale at 2 x.  The baseline is the first-hit path measured in the same run.  Printed, and recorded in DESIGN.md section 14:
    the shares, the MSE over mirror / glass / delta / whole frame of both runs and of the two upscaled frames.

    Asserted: over the pixels whose first hit is the MIRROR the chain-guided display MSE is below the first-hit-guided one.  The
    inequality over all delta pixels fails, and it fails on the glass pixels alone (measured, display MSE, first-hit / chain guides):
    mirror 3.8170e-4 / 3.8108e-4, glass 3.6454e-4 / 6.9313e-4, delta 3.7312e-4 / 5.3710e-4, frame 4.6102e-4 / 4.9156e-4; unfiltered
    2.8224e-4 over the delta pixels.  Why the glass loses: its radiance is a Fresnel MIX of a reflected and a refracted path and
    the chain follows one branch, so the albedo of the refracted floor also demodulates the reflected sky; e = c / d then jumps at
    every checker edge seen through the glass and the filter, stopped by the luminance weight on one side only, smears it.  The
    mirror's margin is thin because most of it reflects the sky, where both kinds of guide are flat."""
    sc = quality_scene()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**QUALITY_CAMERA)
    (w, h), (sw, sh), spp = (320, 180), (160, 90), 16
    mirror, glass = delta_shares(O, sc, QUALITY_CAMERA, w, h)
    delta = mirror | glass
    assert delta.mean() >= 0.05, (mirror.mean(), glass.mean())
    ref, _ = gpu.render(cam, abi.default_render_opts(w, h, 4096, method=abi.RT_METHOD_MIS, seed=99))
    lum = lambda a: F32(0.2126) * a[..., 0] + F32(0.7152) * a[..., 1] + F32(0.0722) * a[..., 2]  # noqa: E731

    def inputs(width, height):
        """colour and variance as rt_render_denoised forms them (two half renders, the variance under first-hit demodulation),
        and both sets of guides"""
        oa = abi.default_render_opts(width, height, spp // 2, method=abi.RT_METHOD_MIS, seed=1)
        ob = abi.default_render_opts(width, height, spp // 2, method=abi.RT_METHOD_MIS, seed=1)
        ob.sample_begin = spp // 2
        a, b = gpu.render(cam, oa)[0], gpu.render(cam, ob)[0]
        o = abi.default_render_opts(width, height, spp, seed=1)
        first = gpu.render_aov(cam, o, channels=("albedo", "normal", "depth"))
        chain = gpu.render_aov_chain(cam, o, channels=("albedo", "normal", "depth", "bounces"))
        d = np.maximum(first["albedo"], F32(1e-3))
        diff = lum(a / d) - lum(b / d)
        return (a + b) * F32(0.5), diff * diff * F32(0.25), first, chain

    color, variance, first, chain = inputs(w, h)
    guides = lambda g: {k: g[k] for k in ("albedo", "normal", "depth")}  # noqa: E731
    out_first = gpu.denoise(color, variance=variance, **guides(first))
    out_chain = gpu.denoise(color, variance=variance, **guides(chain))
    se = {"noisy": _display_se(color, ref), "first": _display_se(out_first, ref), "chain": _display_se(out_chain, ref)}
    # the same pair through rt_upscale at 2 x: filtered at 160 x 90 under each kind of guide, reconstructed under the same kind
    s_color, s_var, s_first, s_chain = inputs(sw, sh)
    up_first = gpu.upscale(gpu.denoise(s_color, variance=s_var, **guides(s_first)), src=guides(s_first), dst=guides(first))
    up_chain = gpu.upscale(gpu.denoise(s_color, variance=s_var, **guides(s_chain)), src=guides(s_chain), dst=guides(chain))
    se["up_first"], se["up_chain"] = _display_se(up_first, ref), _display_se(up_chain, ref)
    print(f"quality scene 320x180x16: mirror share {mirror.mean():.4f} glass share {glass.mean():.4f} "
          f"mean bounces {float(chain['bounces'].mean()):.4f} (over delta pixels {float(chain['bounces'][delta].mean()):.4f})")
    for region, mask in (("mirror", mirror), ("glass", glass), ("delta", delta), ("frame", np.ones_like(delta))):
        print(f"  display MSE over {region}: " + " ".join(f"{k} {float(v[mask].mean()):.4e}" for k, v in se.items()))
    assert se["chain"][mirror].mean() < se["first"][mirror].mean(), (se["chain"][mirror].mean(), se["first"][mirror].mean())
