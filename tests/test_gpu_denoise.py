"""The A-Trous denoiser (rt_denoise, rt_denoise_device, rt_render_denoised) on the GPU: against the float64 checker
(tests/denoise_checker.py), edge cases, determinism, rt_render_denoised against its parts, quality against a converged render,
side effects and graph capture."""
import ctypes as C

import numpy as np
import pytest

import denoise_checker as K
import scenes
from gpu_support import assert_render_unaffected, capture
from post_runners import SCENES, TOL, check_against_checker, device_run, display_mse, rendered_inputs, synthetic

pytestmark = pytest.mark.gpu
abi = scenes.abi

INPUT_SETS = {
    "all": ("albedo", "normal", "depth", "variance"),
    "no_albedo": ("normal", "depth", "variance"),
    "no_normal": ("albedo", "depth", "variance"),
    "no_depth": ("albedo", "normal", "variance"),
    "no_variance": ("albedo", "normal", "depth"),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_gpu_matches_the_checker(hb, name):
    sc, cam_params = SCENES[name]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    for w, h in ((64, 36), (67, 37)):
        full = rendered_inputs(gpu, cam, w, h)
        for set_name, keys in INPUT_SETS.items():
            inputs = {"color": full["color"], **{k: full[k] for k in keys}}
            for it in (1, 5):
                out = gpu.denoise(**inputs, iterations=it)
                ref = check_against_checker(out, inputs, f"{name} {w}x{h} {set_name} iterations={it}", iterations=it)
                if it == 5 and set_name == "all":  # the filter does something
                    assert K.relative_error(full["color"], ref) > 1e-3


@pytest.fixture(scope="module")
def dev_scene(hb):
    sc, cam_params = SCENES["rtweekend1"]()
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (7, 5)])
def test_tiny_frames(hb, dev_scene, w, h):
    gpu, _ = dev_scene
    full = synthetic(h, w, seed=w * 10 + h)
    for keys in INPUT_SETS.values():
        inputs = {"color": full["color"], **{k: full[k] for k in keys}}
        check_against_checker(gpu.denoise(**inputs, iterations=5), inputs, f"{w}x{h} {keys}", iterations=5)


def test_nan_and_inf_pixels_pass_through(hb, dev_scene):
    gpu, _ = dev_scene
    h, w = 24, 40
    full = synthetic(h, w, seed=7)
    for keys in (INPUT_SETS["all"], INPUT_SETS["no_variance"]):
        inputs = {"color": full["color"].copy(), **{k: full[k] for k in keys}}
        inputs["color"][5, 7, 0] = np.nan
        inputs["color"][17, 30, 2] = np.inf
        out = gpu.denoise(**inputs)
        bad = np.zeros((h, w), bool)
        bad[5, 7] = bad[17, 30] = True
        assert np.array_equal(out[bad], inputs["color"][bad], equal_nan=True)
        assert np.isfinite(out[~bad]).all()
        masked = dict(inputs, color=full["color"])
        ref = K.denoise(masked["color"], masked.get("albedo"), masked.get("normal"), masked.get("depth"), masked.get("variance"),
                        exclude=bad)
        assert K.relative_error(out[~bad], ref[~bad]) <= TOL
    v = full["variance"].copy()  # a non-finite variance marks the pixel too
    v[3, 3] = np.inf
    out = gpu.denoise(full["color"], variance=v)
    assert np.array_equal(out[3, 3], full["color"][3, 3])


def test_half_plane_edges_do_not_bleed(hb, dev_scene):
    gpu, _ = dev_scene
    h, w = 32, 48
    c = np.zeros((h, w, 3), np.float32)
    c[:, : w // 2] = (0.9, 0.2, 0.1)
    c[:, w // 2:] = (0.1, 0.3, 0.8)
    var = np.full((h, w), 1e30, np.float32)
    normal = np.zeros((h, w, 3), np.float32)
    normal[:, : w // 2] = (1, 0, 0)
    normal[:, w // 2:] = (0, 1, 0)
    depth = np.zeros((h, w), np.float32)
    depth[:, w // 2:] = 5.0
    for guides in (dict(normal=normal), dict(depth=depth)):
        out = gpu.denoise(c, variance=var, **guides)
        assert np.abs(out - c).max() <= 1e-6 * np.abs(c).max(), guides
    assert np.abs(gpu.denoise(c, variance=var) - c).max() > 0.1  # unguided, they mix


def test_invalid_arguments_on_a_device_scene(hb, dev_scene):
    gpu, _ = dev_scene
    lib = hb.lib()
    c = np.zeros((4, 5, 3), np.float32)
    ins = abi.DenoiseInputs()
    ins.color = c.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros_like(c)
    out_p = out.ctypes.data_as(C.POINTER(C.c_float))
    cases = [(hb.denoise_opts(5, 4, iterations=0), out_p, abi.RT_ERR_INVALID_ARGUMENT),
             (hb.denoise_opts(5, 4, sigma_luminance=float("nan")), out_p, abi.RT_ERR_INVALID_ARGUMENT),
             (hb.denoise_opts(0, 4), out_p, abi.RT_ERR_INVALID_ARGUMENT),
             (hb.denoise_opts(5, 4), ins.color, abi.RT_ERR_INVALID_ARGUMENT),
             (hb.denoise_opts(1 << 16, (1 << 15) + 1), out_p, abi.RT_ERR_UNSUPPORTED)]
    for opts, o, code in cases:
        assert lib.rt_denoise(gpu._h, C.byref(ins), C.byref(opts), o) == code
    o = abi.default_render_opts(16, 9, 3)
    with pytest.raises(hb.RtHipError) as e:
        gpu.render_denoised(dev_scene[1], o)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT


def test_determinism_and_entry_points_agree(hb, dev_scene):
    import torch
    gpu, cam = dev_scene
    w, h = 67, 37
    inputs = rendered_inputs(gpu, cam, w, h)
    a, b = gpu.denoise(**inputs), gpu.denoise(**inputs)
    assert a.tobytes() == b.tobytes()
    opts = hb.denoise_opts(w, h)
    assert device_run(torch, hb, gpu, inputs, opts, 0).tobytes() == a.tobytes()
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    assert device_run(torch, hb, gpu, inputs, opts, side.cuda_stream).tobytes() == a.tobytes()
    no_var = {k: v for k, v in inputs.items() if k != "variance"}
    assert device_run(torch, hb, gpu, no_var, opts, side.cuda_stream).tobytes() == gpu.denoise(**no_var).tobytes()
    sc, _ = SCENES["rtweekend1"]()
    multi = hb.HipScene(sc, devices=[0, 0])
    assert device_run(torch, hb, multi, inputs, opts, 0).tobytes() == a.tobytes()
    assert multi.denoise(**inputs).tobytes() == a.tobytes()


@pytest.mark.parametrize("sample_begin", [0, 6])
@pytest.mark.parametrize("sample_split", [1, 0])
def test_render_denoised_is_its_parts(hb, sample_begin, sample_split):
    sc, cam_params = SCENES["overshadowed"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    w, h, spp = 96, 54, 8
    opts = abi.default_render_opts(w, h, spp, seed=5)
    opts.sample_begin = sample_begin
    opts.sample_split = sample_split
    clean, noisy, rays = gpu.render_denoised(cam, opts)
    halves, half_rays = [], 0
    for begin in (sample_begin, sample_begin + spp // 2):
        o = abi.default_render_opts(w, h, spp // 2, seed=5)
        o.sample_begin = begin
        o.sample_split = sample_split
        img, r = gpu.render(cam, o)
        halves.append(img)
        half_rays += r
    assert noisy.tobytes() == ((halves[0] + halves[1]) * np.float32(0.5)).tobytes()
    assert rays == half_rays
    aov = gpu.render_aov(cam, opts, channels=("albedo", "normal", "depth"))
    var = K.halves_variance(halves[0], halves[1], aov["albedo"])
    assert clean.tobytes() == gpu.denoise(noisy, aov, variance=var).tobytes()
    # and a non-default filter option reaches the filter
    clean3, _, _ = gpu.render_denoised(cam, opts, hb.denoise_opts(0, 0, iterations=3))
    assert clean3.tobytes() == gpu.denoise(noisy, aov, variance=var, iterations=3).tobytes()


QUALITY = {"rtweekend1": 0.5, "overshadowed": 0.7}


@pytest.mark.parametrize("name", list(QUALITY))
def test_quality_against_a_converged_render(hb, name):
    sc, cam_params = SCENES[name]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    w, h = 320, 180
    ref, _ = gpu.render(cam, abi.default_render_opts(w, h, 4096, method=abi.RT_METHOD_MIS, seed=99))
    clean, noisy, _ = gpu.render_denoised(cam, abi.default_render_opts(w, h, 16, method=abi.RT_METHOD_MIS, seed=1))
    mse_noisy, mse_clean = display_mse(noisy, ref), display_mse(clean, ref)
    ratio = mse_clean / mse_noisy
    mean_shift = abs(float(clean.astype(np.float64).mean()) / float(noisy.astype(np.float64).mean()) - 1.0)
    print(f"{name}: display MSE noisy {mse_noisy:.4e} clean {mse_clean:.4e} ratio {ratio:.3f}; mean radiance shift {mean_shift:.4f}")
    assert ratio <= QUALITY[name], (mse_noisy, mse_clean)
    assert mean_shift <= 0.02


def test_no_side_effects_on_render(hb):
    sc, cam_params = SCENES["overshadowed"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)

    def both_calls(opts, img):
        gpu.denoise(img)
        gpu.denoise(img, albedo=np.ones_like(img), variance=np.zeros(img.shape[:2], np.float32))

    assert_render_unaffected(gpu, cam, both_calls)


def test_render_aov_and_denoise_are_graph_capturable(hb):
    import torch
    sc, cam_params = SCENES["all_materials"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    w, h = 160, 90
    opts = abi.default_render_opts(w, h, 8, seed=11)
    dopts = hb.denoise_opts(w, h)
    dev = torch.device("cuda", 0)
    color = torch.zeros(h * w * 3, dtype=torch.float32, device=dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    aov = {k: torch.zeros(h * w * (3 if k != "depth" else 1), dtype=torch.float32, device=dev) for k in ("albedo", "normal", "depth")}
    ws = torch.empty(hb.denoise_workspace_bytes(dopts), dtype=torch.uint8, device=dev)
    out = torch.zeros(h * w * 3, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)

    def launch_all(stream_handle):
        gpu.render_device(cam, opts, color.data_ptr(), rays.data_ptr(), stream_handle)
        gpu.render_aov_device(cam, opts, {k: v.data_ptr() for k, v in aov.items()}, stream=stream_handle)
        gpu.denoise_device({"color": color.data_ptr(), **{k: v.data_ptr() for k, v in aov.items()}}, ws.data_ptr(), out.data_ptr(),
                           dopts, stream=stream_handle)

    with torch.cuda.stream(side):
        launch_all(side.cuda_stream)  # uncaptured (first-use allocations of the render happen here)
    side.synchronize()
    direct = out.cpu().numpy().copy()
    img, _ = gpu.render(cam, opts)
    a = gpu.render_aov(cam, opts, channels=("albedo", "normal", "depth"))
    assert direct.tobytes() == gpu.denoise(img, a).tobytes()
    graph = capture(torch, launch_all, side=side)
    for _ in range(2):
        for t in (color, out, *aov.values()):
            t.fill_(7)
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert out.cpu().numpy().tobytes() == direct.tobytes()


def test_full_frame_1080p(hb):
    sc, cam_params = SCENES["rtweekend1"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    inputs = rendered_inputs(gpu, cam, 1920, 1080, spp=16, seed=1)
    out = gpu.denoise(**inputs, iterations=5)
    check_against_checker(out, inputs, "1080p rtweekend1", iterations=5)
