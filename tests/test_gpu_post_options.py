"""The options of the post-processing stages OFF their defaults on the GPU, one at a time and all at once
(tests/post_options_cases.py), through the host entry and the _device entry of every stage, against the stage's checker given the
same value: under TOL of denoise_checker.relative_error for the denoiser and the temporal filter, bit for bit for the per-pixel
temporal stage, the display and the upscaler.  A kernel that hard-codes a default, or a host wrapper that drops a field of
DevDenoiseParams / DevTemporalParams / DevDisplayParams / DevUpscaleParams, fails here.  That each value changes the checker's
result on the synthetic inputs is held by tests/test_post_options.py; on rendered inputs this file asserts it before comparing."""
import numpy as np
import pytest

import denoise_checker as K
import post_options_cases as P
import scenes
from gpu_support import load_gpu
from post_runners import (GUIDES, SCENES, DeviceDisplay, DeviceRunner, DeviceUpscale, check_against_checker, check_display,
                          check_step, check_upscale, device_run, library_inputs, rendered_inputs, same_state)

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32


def _load(hb, name):
    gpu, cam_params = load_gpu(hb, SCENES, name)
    return gpu, hb.camera_new(**cam_params)


@pytest.fixture(scope="module")
def dev_scene(hb):
    return _load(hb, "rtweekend1")


@pytest.fixture(scope="module")
def denoise_inputs(hb, dev_scene):
    name, w, h = P.DENOISE_RENDERED
    gpu, cam = _load(hb, name)
    return {"synthetic": P.denoise_synthetic(), "rendered": rendered_inputs(gpu, cam, w, h)}


@pytest.mark.parametrize("source", ["synthetic", "rendered"])
@pytest.mark.parametrize("case", P.DENOISE_CASES, ids=[c[0] for c in P.DENOISE_CASES])
def test_denoise_options(hb, dev_scene, denoise_inputs, case, source):
    import torch
    gpu, _ = dev_scene
    name, opts = case
    inputs = denoise_inputs[source]
    h, w = inputs["color"].shape[:2]
    moved = P.denoise_sensitivity(inputs, opts)
    assert moved >= P.SENSITIVITY, f"{name} does nothing on the {source} frame: {moved:.3e}"
    host = gpu.denoise(**inputs, **opts)
    ref = check_against_checker(host, inputs, f"{source} {name} host", **opts)
    dev = device_run(torch, hb, gpu, inputs, hb.denoise_opts(w, h, **opts), 0)
    check_against_checker(dev, inputs, f"{source} {name} device", **opts)
    assert dev.tobytes() == host.tobytes()
    print(f"denoise {source} {name}: moved {moved:.3e}, error {K.relative_error(host, ref):.3e}")


@pytest.mark.parametrize("case", P.TEMPORAL_CASES, ids=[c[0] for c in P.TEMPORAL_CASES])
def test_temporal_options(hb, dev_scene, case):
    import torch
    gpu, _ = dev_scene
    name, kind, frames, opts = case
    w, h = P.TEMPORAL_SIZE if kind == "moving" else P.TEMPORAL_STATIC_SIZE
    run = DeviceRunner(torch, hb, gpu, w, h, iterations=P.TEMPORAL_ITERATIONS, **opts)
    gpu.temporal_reset()
    prev, n_seen = None, set()
    for i in range(frames):
        cam, inputs = P.temporal_camera(hb, kind, i), P.temporal_frame(kind, i)
        out, motion, h_out, h_in = run.step(inputs, cam)
        st = check_step(inputs, cam, prev, h_in, out, motion, h_out, f"{name} frame {i}", iterations=P.TEMPORAL_ITERATIONS, **opts)
        host_out, host_motion = gpu.denoise_temporal(inputs, cam, motion=True, iterations=P.TEMPORAL_ITERATIONS, **opts)
        assert host_out.tobytes() == out.tobytes(), f"{name} frame {i}: host entry"
        assert np.array_equal(host_motion, motion, equal_nan=True), f"{name} frame {i}: host entry, motion"
        n_seen.update(np.unique(st["n"]).tolist())
        prev = cam
    if "max_history" in opts and kind == "static":
        assert max(n_seen) == opts["max_history"] < frames  # the sequence ran into the cap
    elif kind == "moving":
        assert max(n_seen) >= 2 and 1 in n_seen  # taps were accepted and rejected


@pytest.mark.parametrize("case", P.DISPLAY_CASES, ids=[c[0] for c in P.DISPLAY_CASES])
def test_display_options(hb, O, dev_scene, case):
    import torch
    import display_checker as D
    gpu, _ = dev_scene
    name, key, opts = case
    img = P.display_image(key)
    h, w = img.shape[:2]
    for (label, state), (in_off, out_off), fmt in zip(P.DISPLAY_STATES, ((0, 0), (1, 3)), (D.RGBA8, D.RGB8)):
        kw = dict(opts, pixel_format=fmt)
        run = DeviceDisplay(torch, hb, gpu, w, h, in_off, out_off, **kw)
        check_display(O, run, img, state, f"{name} {label} device", **kw)  # bytes, histogram and state
    # the host entry from a zero state
    gpu.display_reset()
    px, hist = gpu.display(img, histogram=True, **opts)
    ref_px, ref_hist, ref_st = D.display(O, img, (F32(0), 0, F32(0)), **opts)
    hs = gpu.display_state()
    assert np.array_equal(px, ref_px) and np.array_equal(hist, ref_hist), f"{name} host"
    assert same_state((F32(hs.ev), hs.frames, F32(hs.metered)), ref_st), f"{name} host: state"


@pytest.fixture(scope="module")
def upscale_inputs(hb):
    name, (w, h), (W, H) = P.UPSCALE_RENDERED
    gpu, cam = _load(hb, name)
    color, src, dst = library_inputs(gpu, cam, w, h, W, H)
    return {"rendered": (color, src, dst, W, H), **{k: make() for k, make in P.UPSCALE_SYNTHETIC.items()}}


@pytest.mark.parametrize("source", ["rendered", *P.UPSCALE_SYNTHETIC])
@pytest.mark.parametrize("case", P.UPSCALE_CASES, ids=[c[0] for c in P.UPSCALE_CASES])
def test_upscale_options(hb, O, dev_scene, upscale_inputs, case, source):
    import torch
    gpu, _ = dev_scene
    name, opts = case
    color, src, dst, W, H = upscale_inputs[source]
    assert P.upscale_differs(O, color, src, dst, W, H, opts), f"{name} does nothing on the {source} frame"
    host_out, host_stage = check_upscale(O, gpu, color, src, dst, W, H, f"{source} {name} host", **opts)
    run = DeviceUpscale(torch, hb, gpu, color, src, dst, W, H, off=1, **opts)
    torch.cuda.synchronize()
    run.launch()
    out, stage = run.read()
    assert out.tobytes() == host_out.tobytes() and stage.tobytes() == host_stage.tobytes(), f"{source} {name} device"


def test_one_call_forms_pass_their_options_on(hb):
    """rt_render_denoised and rt_render_upscaled with every filter and upscale option off its default equal their parts byte for
    byte, and differ from the same calls at the defaults"""
    gpu, cam = _load(hb, "overshadowed")
    (w, h), (W, H), spp = (80, 45), (160, 90), 8
    so, do = abi.default_render_opts(w, h, spp, seed=5), abi.default_render_opts(W, H, spp, seed=5)
    src = gpu.render_aov(cam, so, channels=GUIDES)
    dst = gpu.render_aov(cam, do, channels=GUIDES)
    halves = []
    for begin in (0, spp // 2):
        o = abi.default_render_opts(w, h, spp // 2, seed=5)
        o.sample_begin = begin
        halves.append(gpu.render(cam, o)[0])
    var = K.halves_variance(halves[0], halves[1], src["albedo"])
    clean0, noisy, _ = gpu.render_denoised(cam, so)
    up0, _, _ = gpu.render_upscaled(cam, do, w, h)
    for _, dkw in P.DENOISE_CASES:
        clean, noisy_again, _ = gpu.render_denoised(cam, so, hb.denoise_opts(0, 0, **dkw))
        assert noisy_again.tobytes() == noisy.tobytes()
        assert clean.tobytes() == gpu.denoise(noisy, src, variance=var, **dkw).tobytes(), dkw
        assert clean.tobytes() != clean0.tobytes(), dkw
        for _, ukw in P.UPSCALE_CASES:
            up, up_src, _ = gpu.render_upscaled(cam, do, w, h, hb.denoise_opts(0, 0, **dkw), hb.upscale_opts(0, 0, 0, 0, **ukw))
            assert up_src.tobytes() == clean.tobytes(), (dkw, ukw)
            assert up.tobytes() == gpu.upscale(clean, src=src, dst=dst, **ukw).tobytes(), (dkw, ukw)
            assert up.tobytes() != up0.tobytes(), (dkw, ukw)
    for _, ukw in P.UPSCALE_CASES:  # the upscale options alone, behind the default filter
        up, _, _ = gpu.render_upscaled(cam, do, w, h, None, hb.upscale_opts(0, 0, 0, 0, **ukw))
        assert up.tobytes() == gpu.upscale(clean0, src=src, dst=dst, **ukw).tobytes() and up.tobytes() != up0.tobytes(), ukw
