"""The display stage (rt_display, rt_display_device) on the GPU: bytes, histogram and state against the numpy checker
(tests/display_checker.py) bit for bit over every tone curve x transfer x quantiser x pixel format on rendered frames and at
unaligned sizes and offsets, an adapting AUTO sequence, the identity with rt_output_rgb8_device, the host entry against the device
entry, graph capture (alone and behind render, AOV and the temporal denoiser), side effects and a multi-device head."""
import itertools

import numpy as np
import pytest

import display_checker as D
import scenes
from gpu_support import assert_render_unaffected, capture, load_gpu
from post_runners import SCENES, DeviceDisplay, check_display, same_state, state_tuple

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
FRAME_SCENES = ["rtweekend1", "overshadowed", "all_materials"]


def render(hb, gpu, p, w, h, spp=8, seed=3):
    img, _ = gpu.render(hb.camera_new(**p), abi.default_render_opts(w, h, spp, method=abi.RT_METHOD_MIS, seed=seed))
    return img


@pytest.fixture(scope="module")
def frames(hb):
    out = {}
    for name in FRAME_SCENES:
        gpu, p = load_gpu(hb, SCENES, name)
        out[name] = render(hb, gpu, p, 33, 17)
        gpu.close()
    return out


COMBOS = list(itertools.product(range(4), range(3), range(3), range(3)))


@pytest.mark.parametrize("tonemap,transfer,quantiser,fmt", COMBOS)
def test_every_combination_matches_the_checker(hb, O, frames, tonemap, transfer, quantiser, fmt):
    import torch
    gpu, _ = load_gpu(hb, SCENES, "rtweekend1")
    kw = dict(tonemap=tonemap, transfer=transfer, quantiser=quantiser, pixel_format=fmt, seed=0x1234567890AB, white=3.0, gamma=1.8)
    for name, img in frames.items():
        for (h, w), (in_off, out_off) in itertools.product(((17, 33), (5, 7), (1, 1)), ((0, 0), (1, 3))):
            crop = np.ascontiguousarray(img[:h, :w])
            what = f"{name} {w}x{h} offsets {in_off},{out_off}"
            for label, state, extra in (("zero state", (F32(0), 0, F32(0)), {}),
                                        ("adapting", (F32(1.25), 5, F32(-3.0)), dict(adaptation=0.3)),
                                        ("no state", None, dict(exposure_mode=D.FIXED, exposure_ev=-0.5))):
                run = DeviceDisplay(torch, hb, gpu, w, h, in_off, out_off, **kw, **extra)
                check_display(O, run, crop, state, f"{what} {label}", **kw, **extra)


@pytest.mark.parametrize("kw", [dict(), dict(tonemap="hable", transfer="gamma", quantiser="round", pixel_format="bgra8"),
                                dict(exposure_mode="fixed", tonemap="clamp", transfer="gamma", quantiser="reference",
                                     pixel_format="rgb8"),
                                dict(tonemap="reinhard", transfer="linear", quantiser="dither", pixel_format="rgb8", seed=9)])
def test_1080p(hb, O, kw):
    import torch
    gpu, p = load_gpu(hb, SCENES, "rtweekend1")
    w, h = 1920, 1080
    img = render(hb, gpu, p, w, h, spp=1)
    opts = {k: abi.DISPLAY_ENUMS[k][v] if isinstance(v, str) else v for k, v in kw.items()}
    for in_off, out_off in ((0, 0), (1, 1)):
        run = DeviceDisplay(torch, hb, gpu, w, h, in_off, out_off, **opts)
        check_display(O, run, img, (F32(0.5), 2, F32(0)), f"1080p offsets {in_off},{out_off}", **opts)


def test_auto_sequence_with_a_brightness_step(hb, O):
    import torch
    gpu, p = load_gpu(hb, SCENES, "all_materials")
    w, h = 64, 36
    base = render(hb, gpu, p, w, h, spp=8)
    run = DeviceDisplay(torch, hb, gpu, w, h, adaptation=0.3)
    state, evs = (F32(0), 0, F32(0)), []
    for i in range(8):
        img = base * F32(16.0) if i >= 4 else base
        _, state = check_display(O, run, img, state, f"frame {i}", adaptation=0.3)
        evs.append(float(state[0]))
    assert evs[0] == evs[1] == evs[2] == evs[3]  # snapped at frame 0, then steady
    target = float(D.exposure(D.histogram(base * F32(16.0))[0])[0])
    assert abs(evs[0] - target - 4.0) < 0.2  # 16 x brighter: about 4 EV less
    d = [e - target for e in evs[3:]]
    for k in range(1, 5):  # geometric approach, ratio 1 - adaptation
        assert abs(d[k] / d[k - 1] - 0.7) < 1e-4, (k, d)


def test_device_state_advances_on_the_device(hb, O):
    """no upload between calls: the stage reads back what it wrote"""
    import torch
    gpu, p = load_gpu(hb, SCENES, "overshadowed")
    w, h = 64, 36
    img = render(hb, gpu, p, w, h)
    run = DeviceDisplay(torch, hb, gpu, w, h, adaptation=0.5, exposure_ev=1.0)
    run.upload(img, (F32(-3.0), 7, F32(0)))
    state = (F32(-3.0), 7, F32(0))
    for i in range(4):
        torch.cuda.synchronize()
        run.launch()
        px, hist, st = run.read()
        ref_px, _, state = D.display(O, img, state, adaptation=0.5, exposure_ev=1.0)
        assert np.array_equal(px, ref_px) and same_state(st, state), i
    assert state[1] == 11


@pytest.mark.parametrize("gamma", [2.2, 1.0, 0.5])
def test_identity_with_output_rgb8_device(hb, gamma):
    import torch
    gpu, p = load_gpu(hb, SCENES, "rtweekend1")
    dev = torch.device("cuda", 0)
    frame = render(hb, gpu, p, 64, 36) * F32(3.0)
    for w, h in ((64, 36), (33, 17), (1, 1)):
        img = np.ascontiguousarray(frame[:h, :w])
        img.ravel()[:5] = [np.nan, np.inf, 0.0, -0.0, 1e-40][:img.size]
        if gamma != 0.5 and img.size > 5:
            img.ravel()[5:40:3] *= -1  # negatives: the reference's powf gives NaN (or a negative) unless 1/gamma is even
        if gamma == 1.0 and img.size > 50:
            img.ravel()[50] = -np.inf  # -inf: only for an odd 1/gamma
        run = DeviceDisplay(torch, hb, gpu, w, h, exposure_mode="fixed", tonemap="clamp", transfer="gamma", quantiser="reference",
                            pixel_format="rgb8", gamma=gamma)
        px, _, _ = run(img, None)
        ref = torch.zeros(img.size, dtype=torch.uint8, device=dev)
        gpu.output_rgb8_device(run.src.data_ptr(), img.size, ref.data_ptr(), gamma=gamma)
        torch.cuda.synchronize()
        assert px.tobytes() == ref.cpu().numpy().tobytes(), (w, h)


def test_host_entry_equals_device_entry(hb, O):
    import torch
    gpu, p = load_gpu(hb, SCENES, "all_materials")
    w, h = 48, 27
    imgs = [render(hb, gpu, p, w, h, spp=2 + i, seed=i) * F32(1 + 3 * (i % 2)) for i in range(4)]
    kw = dict(adaptation=0.4, seed=77)
    run = DeviceDisplay(torch, hb, gpu, w, h, **kw)
    gpu.display_reset()
    state = (F32(0), 0, F32(0))
    for i, img in enumerate(imgs):
        host_px, host_hist = gpu.display(img, histogram=True, **kw)
        px, hist, st = run(img, state)
        assert host_px.tobytes() == px.tobytes() and np.array_equal(host_hist, hist), i
        hs = gpu.display_state()
        assert same_state((F32(hs.ev), hs.frames, F32(hs.metered)), st), i
        state = st
    assert gpu.display_state().frames == 4
    # reset: a zero state again
    gpu.display_reset()
    assert gpu.display_state().frames == 0
    first = run(imgs[0], (F32(0), 0, F32(0)))[0]
    assert gpu.display(imgs[0], **kw).tobytes() == first.tobytes() and gpu.display_state().frames == 1
    # a new frame size starts over, and so does going back; a new pixel format at the same size does not
    small = np.ascontiguousarray(imgs[1][:10, :12])
    assert gpu.display(small, **kw).tobytes() == D.display(O, small, (F32(0), 0, F32(0)), **kw)[0].tobytes()
    assert gpu.display(imgs[0], **kw).tobytes() == first.tobytes()
    before = gpu.display_state()
    rgb8 = gpu.display(imgs[2], pixel_format="rgb8", **kw)
    ref, _, _ = D.display(O, imgs[2], (F32(before.ev), before.frames, F32(before.metered)), pixel_format=D.RGB8, **kw)
    assert rgb8.tobytes() == ref.tobytes() and gpu.display_state().frames == 2


def test_graph_replay_equals_eager(hb, O):
    import torch
    gpu, p = load_gpu(hb, SCENES, "overshadowed")
    w, h = 96, 54
    img = render(hb, gpu, p, w, h)
    kw = dict(adaptation=0.5, seed=3)
    start = (F32(2.0), 1, F32(0))
    run = DeviceDisplay(torch, hb, gpu, w, h, **kw)
    eager = []
    run.upload(img, start)
    for _ in range(3):
        torch.cuda.synchronize()
        run.launch()
        eager.append(run.read())
    run.upload(img, start)
    g = capture(torch, lambda stream: run.launch(stream=stream))
    assert state_tuple(run.state.cpu().numpy().view(np.uint32))[1] == 1  # capture ran nothing
    for k in range(3):
        run.out.fill_(0x5A)
        g.replay()
        px, hist, st = run.read()
        assert px.tobytes() == eager[k][0].tobytes() and np.array_equal(hist, eager[k][1]) and same_state(st, eager[k][2]), k
    assert st[1] == 4
    # and the checker agrees with the third
    s = start
    for _ in range(3):
        ref_px, _, s = D.display(O, img, s, **kw)
    assert ref_px.tobytes() == px.tobytes()


def test_frame_graph_render_aov_temporal_display(hb, O):
    """render, AOV, rt_denoise_temporal_device and the display on one stream, captured once, replayed with the checker's bytes"""
    import torch
    gpu, p = load_gpu(hb, SCENES, "all_materials")
    w, h = 160, 90
    dev = torch.device("cuda", 0)
    cam = hb.camera_new(**p)
    ropts = abi.default_render_opts(w, h, 2, seed=11)
    topts = hb.temporal_opts(w, h)
    color = torch.zeros(h * w * 3, dtype=torch.float32, device=dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    aov = {k: torch.zeros(h * w * (3 if k != "depth" else 1), dtype=torch.float32, device=dev) for k in ("albedo", "normal", "depth")}
    hist_buf = torch.zeros(hb.temporal_history_bytes(topts) // 4, dtype=torch.float32, device=dev)
    tws = torch.empty(hb.temporal_workspace_bytes(topts), dtype=torch.uint8, device=dev)
    clean = torch.zeros(h * w * 3, dtype=torch.float32, device=dev)
    disp = DeviceDisplay(torch, hb, gpu, w, h, adaptation=0.3)

    def frame(stream_handle):
        gpu.render_device(cam, ropts, color.data_ptr(), rays.data_ptr(), stream_handle)
        gpu.render_aov_device(cam, ropts, {k: v.data_ptr() for k, v in aov.items()}, stream=stream_handle)
        gpu.denoise_temporal_device({"color": color.data_ptr(), **{k: v.data_ptr() for k, v in aov.items()}}, cam, None, 0,
                                    hist_buf.data_ptr(), tws.data_ptr(), clean.data_ptr(), topts, stream=stream_handle)
        gpu.display_device(clean.data_ptr(), disp.opts, disp.state.data_ptr(), disp.ws.data_ptr(), disp.out.data_ptr(),
                           disp.hist.data_ptr(), stream=stream_handle)

    g = capture(torch, frame)
    state = (F32(0), 0, F32(0))
    for k in range(2):
        clean.fill_(7)
        g.replay()
        px, hist, st = disp.read()
        frame_f32 = clean.cpu().numpy().reshape(h, w, 3)
        ref_px, ref_hist, state = D.display(O, frame_f32, state, adaptation=0.3)
        assert px.tobytes() == ref_px.tobytes() and np.array_equal(hist, ref_hist) and same_state(st, state), k
    assert st[1] == 2


def test_no_side_effects_on_render(hb):
    gpu, p = load_gpu(hb, SCENES, "overshadowed")
    cam = hb.camera_new(**p)

    def both_calls(opts, img):
        gpu.display(img)
        gpu.display(img, tonemap="hable", pixel_format="rgb8")

    assert_render_unaffected(gpu, cam, both_calls)


def test_multi_device_head_runs_on_the_first_device(hb):
    single, p = load_gpu(hb, SCENES, "rtweekend1")
    multi, _ = load_gpu(hb, SCENES, "rtweekend1", devices=[0, 0])
    img = render(hb, single, p, 96, 54)
    for i in range(3):
        a = multi.display(img * F32(1 + i), adaptation=0.5)
        b = single.display(img * F32(1 + i), adaptation=0.5)
        assert a.tobytes() == b.tobytes(), i
    assert multi.display_state().frames == single.display_state().frames == 3
