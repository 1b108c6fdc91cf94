"""Temporal accumulation with camera reprojection (rt_denoise_temporal, rt_denoise_temporal_device) on the GPU: per-step exactness
against the float32 checker (tests/temporal_checker.py) over camera paths, the no-history identity with rt_denoise, the host and
device entries against each other, invalid pixels, graph capture, side effects, a 1080p step, a multi-device head and quality
against a converged render."""
import numpy as np
import pytest

import scenes
from gpu_support import assert_render_unaffected, capture, load_gpu
from post_runners import SCENES, DeviceRunner, bits_equal, check_step, display_mse

pytestmark = pytest.mark.gpu
abi = scenes.abi


def path_camera(hb, p, i, orbit_deg=1.5, dolly=0.01):
    """frame i of an orbit about the look-at point (orbit_deg per frame about the camera's vup) plus a dolly towards it"""
    o, at = np.array(p["origin"], np.float64), np.array(p["lookat"], np.float64)
    k = np.array(p["vup"], np.float64)
    k /= np.linalg.norm(k)
    t = np.radians(orbit_deg * i)
    r = o - at
    r = r * np.cos(t) + np.cross(k, r) * np.sin(t) + k * np.dot(k, r) * (1 - np.cos(t))  # Rodrigues
    return hb.camera_new(**dict(p, origin=tuple(at + r * (1.0 - dolly * i))))


def frame_inputs(gpu, cam, w, h, spp, sample_begin, seed=3):
    opts = abi.default_render_opts(w, h, spp, method=abi.RT_METHOD_MIS, seed=seed)
    opts.sample_begin = sample_begin
    color, _ = gpu.render(cam, opts)
    aov = gpu.render_aov(cam, opts, channels=("albedo", "normal", "depth"))
    return dict(color=color, **aov)


PATH_SCENES = ["rtweekend1", "overshadowed", "all_materials", "structured_meshes", "random_everything_1"]


@pytest.mark.parametrize("name", PATH_SCENES)
def test_every_step_matches_the_checker(hb, name):
    import torch
    gpu, p = load_gpu(hb, SCENES, name)
    for w, h in ((160, 90), (320, 180)):
        run = DeviceRunner(torch, hb, gpu, w, h)
        begin, prev = 0, None
        n_max = 0
        for i in range(6):
            cam = path_camera(hb, p, i)
            spp = 2 + i % 3
            inputs = frame_inputs(gpu, cam, w, h, spp, begin)
            begin += spp
            out, motion, h_out, h_in = run.step(inputs, cam)
            st = check_step(inputs, cam, prev, h_in, out, motion, h_out, f"{name} {w}x{h} frame {i}")
            n_max = max(n_max, float(st["n"].max()))
            prev = cam
        assert n_max == 6  # some pixels kept their history all the way


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("name", list(SCENES))
def test_no_history_is_rt_denoise(hb, name, iterations):
    import torch
    gpu, p = load_gpu(hb, SCENES, name)
    cam = hb.camera_new(**p)
    for w, h in ((64, 36), (67, 37)):
        inputs = frame_inputs(gpu, cam, w, h, 4, 0)
        plain = gpu.denoise(**inputs, iterations=iterations)
        gpu.temporal_reset()
        assert gpu.denoise_temporal(inputs, cam, iterations=iterations).tobytes() == plain.tobytes()
        run = DeviceRunner(torch, hb, gpu, w, h, iterations=iterations)
        out, motion, h_out, _ = run.step(inputs, cam)
        assert out.tobytes() == plain.tobytes() and np.isnan(motion).all()
        no_normal = {k: v for k, v in inputs.items() if k != "normal"}
        gpu.temporal_reset()
        assert gpu.denoise_temporal(no_normal, cam, iterations=iterations).tobytes() == \
            gpu.denoise(**no_normal, iterations=iterations).tobytes()


def test_host_and_device_entries_agree(hb):
    import torch
    gpu, p = load_gpu(hb, SCENES, "all_materials")
    w, h = 96, 54
    run = DeviceRunner(torch, hb, gpu, w, h)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    gpu.temporal_reset()
    frames = []
    for i in range(4):
        cam = path_camera(hb, p, i)
        inputs = frame_inputs(gpu, cam, w, h, 2, 2 * i)
        frames.append((inputs, cam))
        host_out, host_motion = gpu.denoise_temporal(inputs, cam, motion=True)
        run.upload(inputs)
        torch.cuda.synchronize()
        run.launch(cam, stream=side.cuda_stream)
        side.synchronize()
        assert host_out.tobytes() == run.out.cpu().numpy().tobytes(), i
        assert bits_equal(host_motion.ravel(), run.motion.cpu().numpy()), i
    # reset: the next call has no history
    inputs, cam = frames[1]
    fresh = gpu.denoise(**inputs)
    gpu.temporal_reset()
    out, motion = gpu.denoise_temporal(inputs, cam, motion=True)
    assert out.tobytes() == fresh.tobytes() and np.isnan(motion).all()
    with_history = gpu.denoise_temporal(inputs, cam)
    assert with_history.tobytes() != fresh.tobytes()
    # a new frame size starts over, and so does going back
    small = frame_inputs(gpu, cam, 64, 36, 2, 0)
    assert gpu.denoise_temporal(small, cam).tobytes() == gpu.denoise(**small).tobytes()
    assert gpu.denoise_temporal(inputs, cam).tobytes() == fresh.tobytes()


def test_nan_and_inf_pixels(hb):
    import torch
    gpu, p = load_gpu(hb, SCENES, "rtweekend1")
    w, h = 64, 36
    cam = hb.camera_new(**p)
    run = DeviceRunner(torch, hb, gpu, w, h)
    inputs = frame_inputs(gpu, cam, w, h, 4, 0)
    bad = dict(inputs, color=inputs["color"].copy())
    bad["color"][5, 7, 0] = np.nan
    bad["color"][17, 30, 2] = np.inf
    out, motion, h_out, h_in = run.step(bad, cam)
    check_step(bad, cam, None, h_in, out, motion, h_out, "frame 0")
    for y, x in ((5, 7), (17, 30)):
        assert np.array_equal(out[y, x], bad["color"][y, x], equal_nan=True)
        assert h_out[0, y, x, 3] == 0 and not h_out[0, y, x, :3].any() and not h_out[2, y, x].any()
    assert np.isfinite(np.delete(out.reshape(-1, 3), [5 * w + 7, 17 * w + 30], axis=0)).all()
    inputs2 = frame_inputs(gpu, cam, w, h, 4, 4)
    out, motion, h_out, h_in = run.step(inputs2, cam)
    st = check_step(inputs2, cam, cam, h_in, out, motion, h_out, "frame 1")
    assert st["n"][5, 7] == 1 and st["n"][17, 30] == 1  # not their own taps: the history starts over there
    assert (st["n"] == 2).mean() > 0.9


def test_ping_pong_graphs_equal_eager(hb):
    import torch
    gpu, p = load_gpu(hb, SCENES, "all_materials")
    w, h = 160, 90
    dev = torch.device("cuda", 0)
    cams = [path_camera(hb, p, 0), path_camera(hb, p, 1)]
    opts = abi.default_render_opts(w, h, 2, seed=11)
    run = DeviceRunner(torch, hb, gpu, w, h)
    color = torch.zeros(h * w * 3, dtype=torch.float32, device=dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    aov = {k: torch.zeros(h * w * (3 if k != "depth" else 1), dtype=torch.float32, device=dev) for k in ("albedo", "normal", "depth")}
    run.t = {"color": color, **aov}
    side = torch.cuda.Stream(device=dev)

    def frame(cam, stream_handle):
        gpu.render_device(cam, opts, color.data_ptr(), rays.data_ptr(), stream_handle)
        gpu.render_aov_device(cam, opts, {k: v.data_ptr() for k, v in aov.items()}, stream=stream_handle)
        run.launch(cam, stream=stream_handle)

    # eager: frame 0 without history into hist[0], then cams[1] (0 -> 1), cams[0] (1 -> 0), ... recorded
    with torch.cuda.stream(side):
        frame(cams[0], side.cuda_stream)
    side.synchronize()
    eager = []
    for k in range(4):
        with torch.cuda.stream(side):
            frame(cams[(k + 1) % 2], side.cuda_stream)
        side.synchronize()
        eager.append(run.out.cpu().numpy().copy())
    # graphs: A = (cams[1], history 0 -> 1), B = (cams[0], history 1 -> 0), captured after the same first frame
    run.cur, run.prev = -1, None
    with torch.cuda.stream(side):
        frame(cams[0], side.cuda_stream)
    side.synchronize()
    graphs = []
    for k in range(2):
        graphs.append(capture(torch, lambda stream: frame(cams[(k + 1) % 2], stream), side=side))
    assert run.cur == 0  # capture launched nothing, but the runner's ping-pong went round once
    for k in range(4):
        run.out.fill_(7)
        torch.cuda.synchronize(dev)
        graphs[k % 2].replay()
        torch.cuda.synchronize(dev)
        assert run.out.cpu().numpy().tobytes() == eager[k].tobytes(), k


def test_no_side_effects_on_render(hb):
    gpu, p = load_gpu(hb, SCENES, "overshadowed")
    cam = hb.camera_new(**p)

    def aov_and_two_frames(opts, img):
        aov = gpu.render_aov(cam, opts, channels=("albedo", "normal", "depth"))
        gpu.denoise_temporal(img, cam, aov)
        gpu.denoise_temporal(img, path_camera(hb, p, 1), aov, motion=True)

    assert_render_unaffected(gpu, cam, aov_and_two_frames)


def test_full_frame_1080p_with_motion(hb):
    import torch
    gpu, p = load_gpu(hb, SCENES, "rtweekend1")
    w, h = 1920, 1080
    run = DeviceRunner(torch, hb, gpu, w, h)
    prev = None
    for i in range(2):
        cam = path_camera(hb, p, i, orbit_deg=0.5, dolly=0.0)
        inputs = frame_inputs(gpu, cam, w, h, 2, 2 * i)
        out, motion, h_out, h_in = run.step(inputs, cam)
        st = check_step(inputs, cam, prev, h_in, out, motion, h_out, f"1080p frame {i}")
        prev = cam
    assert (st["n"] == 2).mean() > 0.9 and np.nanmax(np.abs(motion)) > 1.0


def test_multi_device_head_runs_on_the_first_device(hb):
    single, p = load_gpu(hb, SCENES, "rtweekend1")
    multi, _ = load_gpu(hb, SCENES, "rtweekend1", devices=[0, 0])
    w, h = 96, 54
    for i in range(3):
        cam = path_camera(hb, p, i)
        inputs = frame_inputs(single, cam, w, h, 2, 2 * i)
        assert multi.denoise_temporal(inputs, cam).tobytes() == single.denoise_temporal(inputs, cam).tobytes(), i


def _quality(hb, name, orbit_deg, frames=8, spp=2, w=320, h=180):
    gpu, p = load_gpu(hb, SCENES, name)
    gpu.temporal_reset()
    for i in range(frames):
        cam = path_camera(hb, p, i, orbit_deg=orbit_deg, dolly=0.0)
        inputs = frame_inputs(gpu, cam, w, h, spp, spp * i, seed=1)
        temporal = gpu.denoise_temporal(inputs, cam)
    single = gpu.denoise(**inputs)
    ref, _ = gpu.render(cam, abi.default_render_opts(w, h, 4096, method=abi.RT_METHOD_MIS, seed=99))
    mse_t, mse_s = display_mse(temporal, ref), display_mse(single, ref)
    shift = abs(float(temporal.astype(np.float64).mean()) / float(ref.astype(np.float64).mean()) - 1.0)
    print(f"{name} orbit {orbit_deg} deg/frame: display MSE single-frame {mse_s:.4e} temporal {mse_t:.4e} "
          f"ratio {mse_t / mse_s:.3f}; mean radiance shift {shift:.4f}")
    return mse_t / mse_s, shift


@pytest.mark.parametrize("name", ["rtweekend1", "overshadowed"])
def test_quality_static_camera(hb, name):
    """accumulation must beat the single-frame filter; the 0.6x first estimated is NOT met (0.76x and 0.92x
    measured -- the filter's variance is that of one frame, so its bias, which accumulation does not reduce, dominates)"""
    ratio, shift = _quality(hb, name, 0.0)
    assert ratio < 1.0 and shift <= 0.02


@pytest.mark.parametrize("name", ["rtweekend1", "overshadowed"])
def test_quality_orbit(hb, name):
    ratio, shift = _quality(hb, name, 0.5)
    assert ratio <= 1.0 and shift <= 0.02
