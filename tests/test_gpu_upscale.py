"""AOV-guided upscaling (rt_upscale, rt_upscale_device, rt_render_upscaled) on the GPU: frame AND stage map against the numpy checker
(tests/upscale_checker.py) bit for bit with inputs from the library itself, every subset of guides, ratios 2, 1.5, 3, 1 and an
anisotropic one, sizes off the tile grid, 960 x 540 -> 1920 x 1080; an input built so that every stage value occurs; unaligned
buffers; host entry = device entry; rt_render_upscaled = its parts; NaN / inf pixels; graph replay; side effects; a multi-device
head; quality against a converged render."""
import itertools
import time

import numpy as np
import pytest

import scenes
from gpu_support import assert_render_unaffected, capture, load_gpu
from post_runners import GUIDES, SCENES, STAGES_SEEN, DeviceUpscale, check_upscale, display_mse, library_inputs

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
SUBSETS = [tuple(g for g, on in zip(GUIDES, bits) if on) for bits in itertools.product((False, True), repeat=3)]


def _load(hb, name, devices=None):
    gpu, cam_params = load_gpu(hb, SCENES, name, devices)
    return gpu, hb.camera_new(**cam_params)


def pick(guides, keys):
    return {k: guides[k] for k in keys}


RATIOS = [((64, 36), (128, 72)), ((64, 36), (96, 54)), ((64, 36), (192, 108)), ((64, 36), (64, 36)), ((67, 37), (131, 40))]


@pytest.mark.parametrize("name", list(SCENES))
def test_gpu_matches_the_checker_bit_for_bit(hb, O, name):
    gpu, cam = _load(hb, name)
    for (w, h), (W, H) in RATIOS:
        color, src, dst = library_inputs(gpu, cam, w, h, W, H)
        subsets = SUBSETS if (W, H) in ((128, 72), (131, 40)) else [(), GUIDES]
        for keys in subsets:
            check_upscale(O, gpu, color, pick(src, keys), pick(dst, keys), W, H, f"{name} {w}x{h} -> {W}x{H} guides {keys}")
        check_upscale(O, gpu, color, src, dst, W, H, f"{name} {w}x{h} -> {W}x{H} options", sigma_normal=4.0, depth_tolerance=0.02)


def test_960x540_to_1080p(hb, O):
    gpu, cam = _load(hb, "rtweekend1")
    color, src, dst = library_inputs(gpu, cam, 960, 540, 1920, 1080, spp=4, seed=1)
    _, stage = check_upscale(O, gpu, color, src, dst, 1920, 1080, "960x540 -> 1920x1080")
    share = np.bincount(stage.ravel(), minlength=4) / stage.size
    print(f"rtweekend1 960x540 -> 1920x1080: stage shares 0..3 = {share.round(6).tolist()}")
    assert share[1] > 0.9


def every_stage_input(h=40, w=56, H=80, W=112):
    """built so that every stage value occurs: a block of invalid source pixels (stage 0 in its middle, stage 2 at its rim), and one
    source pixel that alone has the depth and normal of a destination region three source pixels wide (stage 1 in its bilinear
    cell, 2 in the ring of the 4 x 4 window, 3 beyond)"""
    rng = np.random.default_rng(21)
    color = rng.uniform(0.2, 2.0, (h, w, 3)).astype(F32)
    color[20:30, 30:40] = np.nan
    color[3, 3] = (np.inf, 1.0, 1.0)
    ys = (np.arange(H) + 0.5) / (H - 1) * (h - 1) - 0.5
    xs = (np.arange(W) + 0.5) / (W - 1) * (w - 1) - 0.5
    region = (np.abs(xs[None, :] - 13) < 3.2) & (np.abs(ys[:, None] - 9) < 3.2)
    up, right = np.array([0, 1, 0], F32), np.array([1, 0, 0], F32)
    zs, ns = np.full((h, w), 2.0, F32), np.tile(right, (h, w, 1))
    zs[9, 13], ns[9, 13] = 1.0, up
    src = dict(albedo=rng.uniform(0.1, 1.0, (h, w, 3)).astype(F32), normal=ns, depth=zs)
    dst = dict(albedo=rng.uniform(0.1, 1.0, (H, W, 3)).astype(F32), normal=np.where(region[..., None], up, right).astype(F32),
               depth=np.where(region, F32(1.0), F32(2.0)).astype(F32))
    return color, src, dst, W, H


def test_every_stage_value_by_construction(hb, O):
    gpu, _ = _load(hb, "rtweekend1")
    color, src, dst, W, H = every_stage_input()
    for keys in SUBSETS:
        _, stage = check_upscale(O, gpu, color, pick(src, keys), pick(dst, keys), W, H, f"constructed, guides {keys}")
        assert np.isfinite(gpu.upscale(color, src=pick(src, keys), dst=pick(dst, keys) or (H, W))).all()
        if "depth" in keys or "normal" in keys:
            assert set(np.unique(stage)) == {0, 1, 2, 3}, keys
        else:
            assert set(np.unique(stage)) == {0, 1, 2}, keys


def test_nan_and_inf_pixels_in_a_rendered_frame(hb, O):
    gpu, cam = _load(hb, "all_materials")
    color, src, dst = library_inputs(gpu, cam, 64, 36, 128, 72)
    color = color.copy()
    color[5, 7, 0] = np.nan
    color[5, 8, 1] = np.inf
    color[20, 30, 2] = -np.inf
    color[10:16, 40:46] = np.nan
    color[35, 63] = np.nan  # a corner: its clamped copies are invalid too
    for keys in ((), GUIDES):
        out, stage = check_upscale(O, gpu, color, pick(src, keys), pick(dst, keys), 128, 72, f"non-finite pixels, guides {keys}")
        assert np.isfinite(out).all() and (out[stage == 0] == 0).all() and (stage == 0).any()


@pytest.mark.parametrize("sizes", [((67, 37), (131, 75)), ((64, 36), (128, 72))])
def test_device_entry_unaligned_buffers_and_host_entry(hb, O, sizes):
    import torch
    (w, h), (W, H) = sizes
    gpu, cam = _load(hb, "overshadowed")
    color, src, dst = library_inputs(gpu, cam, w, h, W, H)
    for keys in ((), ("albedo",), GUIDES):
        s, d = pick(src, keys), pick(dst, keys)
        host_out, host_stage = check_upscale(O, gpu, color, s, d, W, H, f"host {keys}")
        for off in (0, 1, 3):
            run = DeviceUpscale(torch, hb, gpu, color, s, d, W, H, off=off)
            torch.cuda.synchronize()
            run.launch()
            out, stage = run.read()
            assert out.tobytes() == host_out.tobytes() and stage.tobytes() == host_stage.tobytes(), (keys, off)
        run = DeviceUpscale(torch, hb, gpu, color, s, d, W, H)  # no stage map asked for: the buffer stays untouched
        torch.cuda.synchronize()
        run.launch(with_stage=False)
        out, stage = run.read()
        assert out.tobytes() == host_out.tobytes() and (stage == 0x5A).all()
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    run = DeviceUpscale(torch, hb, gpu, color, src, dst, W, H, off=1)
    torch.cuda.synchronize()
    run.launch(stream=side.cuda_stream)
    assert run.read()[0].tobytes() == host_out.tobytes()


@pytest.mark.parametrize("sample_begin,sample_split", [(0, 1), (6, 0)])
def test_render_upscaled_is_its_parts(hb, sample_begin, sample_split):
    gpu, cam = _load(hb, "overshadowed")
    (w, h), (W, H), spp = (80, 45), (160, 90), 8
    opts = abi.default_render_opts(W, H, spp, seed=5)
    opts.sample_begin, opts.sample_split = sample_begin, sample_split
    out, out_src, rays = gpu.render_upscaled(cam, opts, w, h)
    so = abi.default_render_opts(w, h, spp, seed=5)
    so.sample_begin, so.sample_split = sample_begin, sample_split
    clean, _, src_rays = gpu.render_denoised(cam, so)
    assert out_src.tobytes() == clean.tobytes() and rays == src_rays
    src = gpu.render_aov(cam, so, channels=GUIDES)
    dst = gpu.render_aov(cam, opts, channels=GUIDES)
    assert out.tobytes() == gpu.upscale(clean, src=src, dst=dst).tobytes()
    # non-default options of both stages reach them
    out2, src2, _ = gpu.render_upscaled(cam, opts, w, h, hb.denoise_opts(0, 0, iterations=3), hb.upscale_opts(0, 0, 0, 0, sigma_normal=4.0))
    clean3, _, _ = gpu.render_denoised(cam, so, hb.denoise_opts(0, 0, iterations=3))
    assert src2.tobytes() == clean3.tobytes() and src2.tobytes() != clean.tobytes()
    assert out2.tobytes() == gpu.upscale(clean3, src=src, dst=dst, sigma_normal=4.0).tobytes() and out2.tobytes() != out.tobytes()
    # 1 : 1 and a call after a larger one (the scene's buffer is reused)
    same, same_src, _ = gpu.render_upscaled(cam, so, w, h)
    assert same_src.tobytes() == clean.tobytes() and same.tobytes() == gpu.upscale(clean, src=src, dst=src).tobytes()


def test_invalid_arguments_on_a_device_scene(hb):
    gpu, cam = _load(hb, "rtweekend1")
    c = np.zeros((9, 16, 3), F32)
    for kw, code in ((dict(dst=(8, 16)), abi.RT_ERR_UNSUPPORTED), (dict(dst=(18, 32), sigma_normal=0.0), abi.RT_ERR_INVALID_ARGUMENT),
                     (dict(src=dict(depth=np.ones((9, 16), F32)), dst=(18, 32)), abi.RT_ERR_INVALID_ARGUMENT)):
        with pytest.raises(hb.RtHipError) as e:
            gpu.upscale(c, **kw)
        assert e.value.code == code, kw
    with pytest.raises(hb.RtHipError) as e:
        gpu.render_upscaled(cam, abi.default_render_opts(32, 18, 3), 16, 9)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(hb.RtHipError) as e:
        gpu.render_upscaled(cam, abi.default_render_opts(32, 18, 4), 33, 9)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED


def test_graph_replay_equals_eager(hb):
    """render, AOVs at both sizes, the filter and the upscale on one stream, captured from the upscale's FIRST call, replayed"""
    import torch
    gpu, cam = _load(hb, "all_materials")
    (w, h), (W, H) = (80, 45), (160, 90)
    dev = torch.device("cuda", 0)
    so, do = abi.default_render_opts(w, h, 4, seed=11), abi.default_render_opts(W, H, 4, seed=11)
    dopts, uopts = hb.denoise_opts(w, h), hb.upscale_opts(w, h, W, H)
    f = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)  # noqa: E731
    color, clean, rays = f(h * w * 3), f(h * w * 3), torch.zeros(1, dtype=torch.int64, device=dev)
    src = {k: f(h * w * (3 if k != "depth" else 1)) for k in GUIDES}
    dst = {k: f(H * W * (3 if k != "depth" else 1)) for k in GUIDES}
    ws = torch.empty(hb.denoise_workspace_bytes(dopts), dtype=torch.uint8, device=dev)
    out, stage = f(H * W * 3), torch.zeros(H * W, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)

    def frame(sh, upscale=True):
        gpu.render_device(cam, so, color.data_ptr(), rays.data_ptr(), sh)
        gpu.render_aov_device(cam, so, {k: v.data_ptr() for k, v in src.items()}, stream=sh)
        gpu.render_aov_device(cam, do, {k: v.data_ptr() for k, v in dst.items()}, stream=sh)
        gpu.denoise_device({"color": color.data_ptr(), **{k: v.data_ptr() for k, v in src.items()}}, ws.data_ptr(), clean.data_ptr(),
                           dopts, stream=sh)
        if upscale:
            gpu.upscale_device({"color": clean.data_ptr(), **{"src_" + k: v.data_ptr() for k, v in src.items()},
                                **{"dst_" + k: v.data_ptr() for k, v in dst.items()}}, out.data_ptr(), uopts, stage.data_ptr(), stream=sh)

    with torch.cuda.stream(side):
        frame(side.cuda_stream, upscale=False)  # the render's and the AOV pass's first-use allocations; the upscale has none
    side.synchronize()
    g = capture(torch, frame, side=side)
    assert (out.cpu().numpy() == 0).all()  # capture ran nothing
    eager = gpu.upscale(clean.cpu().numpy().reshape(h, w, 3), src={k: v.cpu().numpy().reshape((h, w, 3) if k != "depth" else (h, w))
                                                                   for k, v in src.items()},
                        dst={k: v.cpu().numpy().reshape((H, W, 3) if k != "depth" else (H, W)) for k, v in dst.items()}, stage=True)
    for _ in range(2):
        for t in (color, clean, out, *src.values(), *dst.values()):
            t.fill_(7)
        stage.fill_(9)
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        assert out.cpu().numpy().tobytes() == eager[0].tobytes() and stage.cpu().numpy().tobytes() == eager[1].tobytes()


def test_no_side_effects_on_render(hb):
    gpu, cam = _load(hb, "overshadowed")

    def aov_and_both_calls(opts, img):
        aov = gpu.render_aov(cam, opts, channels=GUIDES)
        gpu.upscale(img, dst=(108, 192))
        gpu.upscale(img, src=aov, dst=aov, stage=True)

    assert_render_unaffected(gpu, cam, aov_and_both_calls)


def test_multi_device_head_runs_on_the_first_device(hb):
    import torch
    single, cam = _load(hb, "rtweekend1")
    multi, _ = _load(hb, "rtweekend1", devices=[0, 0])
    (w, h), (W, H) = (64, 36), (128, 72)
    color, src, dst = library_inputs(single, cam, w, h, W, H)
    a, sa = single.upscale(color, src=src, dst=dst, stage=True)
    b, sb = multi.upscale(color, src=src, dst=dst, stage=True)
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()
    run = DeviceUpscale(torch, hb, multi, color, src, dst, W, H)
    torch.cuda.synchronize()
    run.launch()
    assert run.read()[0].tobytes() == a.tobytes()
    opts = abi.default_render_opts(W, H, 4, seed=4)
    assert multi.render_upscaled(cam, opts, w, h)[0].tobytes() == single.render_upscaled(cam, opts, w, h)[0].tobytes()


QUALITY_SCENES = ["rtweekend1", "overshadowed", "all_materials"]  # all_materials: checker, Perlin, image and lerp textures in the albedo


@pytest.mark.parametrize("name", QUALITY_SCENES)
def test_quality_against_a_converged_render(hb, name):
    """The protocol of the denoiser's quality test: display-space MSE against a 4096-pass render at 320 x 180; rt_render_upscaled from
    160 x 90 at 16 MIS passes.  Asserted: the guided result beats the unguided call on the same source frame, and its mean is within
    2 % of the mean of the source frame it was made from.  Measured figures: DESIGN.md section 13."""
    gpu, cam = _load(hb, name)
    (w, h), (W, H) = (160, 90), (320, 180)
    ref, _ = gpu.render(cam, abi.default_render_opts(W, H, 4096, method=abi.RT_METHOD_MIS, seed=99))
    opts = abi.default_render_opts(W, H, 16, method=abi.RT_METHOD_MIS, seed=1)
    guided, source, _ = gpu.render_upscaled(cam, opts, w, h)
    t0 = time.perf_counter()
    gpu.render_upscaled(cam, opts, w, h)
    t_up = time.perf_counter() - t0
    plain = gpu.upscale(source, dst=(H, W))
    mse_guided, mse_plain = display_mse(guided, ref), display_mse(plain, ref)
    ratio = mse_guided / mse_plain
    mean_shift = abs(float(guided.astype(np.float64).mean()) / float(source.astype(np.float64).mean()) - 1.0)
    # not asserted: the equal-cost alternative, the full-size frame with a quarter of the passes
    o4 = abi.default_render_opts(W, H, 4, method=abi.RT_METHOD_MIS, seed=1)
    full4, _, _ = gpu.render_denoised(cam, o4)
    t0 = time.perf_counter()
    gpu.render_denoised(cam, o4)
    t_full = time.perf_counter() - t0
    full16, _, _ = gpu.render_denoised(cam, opts)
    print(f"{name}: display MSE guided {mse_guided:.4e} unguided {mse_plain:.4e} ratio {ratio:.3f}; mean shift {mean_shift:.4f}; "
          f"equal cost: 320x180 @ 4 passes denoised MSE {display_mse(full4, ref):.4e} in {t_full * 1e3:.2f} ms, "
          f"160x90 @ 16 upscaled in {t_up * 1e3:.2f} ms; 320x180 @ 16 passes denoised MSE {display_mse(full16, ref):.4e}")
    assert ratio < 1.0, (mse_guided, mse_plain)
    assert mean_shift <= 0.02


def test_zz_every_stage_value_occurred():
    """runs last in this module: the union of every stage map checked above"""
    assert STAGES_SEEN == {0, 1, 2, 3}, STAGES_SEEN
