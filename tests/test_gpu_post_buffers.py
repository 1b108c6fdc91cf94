"""The scene-owned device buffers behind the blocking post-processing entry points: every blocking stage on ONE scene at 13 x 11,
then 45 x 27 (its buffer grows), then 7 x 5 (a smaller frame in the larger buffer), each result bit for bit the stage's _device
entry on torch-allocated buffers, so that the wrapper's internal layout is the only difference between the two sides; the display's
state carried across a growth of its buffer; and the one-call composites that share the denoiser's buffer, interleaved on one scene,
each output bit for bit the same call made first on a fresh scene.  The sizes are odd: 12 n and 4 n are no multiples of 16."""
import ctypes as C

import numpy as np
import pytest

import scenes
from gpu_support import assert_same_bits, load_gpu
from post_runners import SCENES, DeviceDisplay, DeviceRunner, DeviceUpscale, device_run, rendered_inputs
from test_gpu_bloom import DeviceBloom, hdr_frame
from test_gpu_dof import DeviceDof, depth_plane

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
SPP = 2
FRAMES = [(13, 11), (45, 27), (7, 5)]
UPSCALES = [((7, 5), (13, 9)), ((13, 11), (45, 27)), ((7, 5), (13, 9))]
GUIDES = ("albedo", "normal", "depth")


def fresh(hb):
    gpu, cam_params = load_gpu(hb, SCENES, "all_materials")
    return gpu, hb.camera_new(**cam_params)


@pytest.fixture(scope="module")
def ref(hb):
    """the scene the _device side runs on, and what it rendered per frame size (computed once, never written)"""
    gpu, cam = fresh(hb)
    cache = {}

    def inputs(w, h):
        if (w, h) not in cache:
            cache[w, h] = rendered_inputs(gpu, cam, w, h, spp=SPP)
        return cache[w, h]

    return gpu, cam, inputs


@pytest.fixture()
def gpu(hb):
    """the scene under test: a new one per test, so that the first frame allocates and the second grows"""
    g, _ = fresh(hb)
    yield g
    g.close()


def to_dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def test_denoise(hb, gpu, ref):
    import torch
    rgpu, _, inputs = ref
    for w, h in FRAMES:
        full = inputs(w, h)
        for names in (("color", *GUIDES, "variance"), ("color", *GUIDES), ("color",)):
            ins = {k: full[k] for k in names}
            want = device_run(torch, hb, rgpu, ins, hb.denoise_opts(w, h), 0)
            assert_same_bits(gpu.denoise(**ins), want, f"denoise {w}x{h} {names}", nan_equal=True)


def test_denoise_temporal_two_frames(hb, gpu, ref):
    import torch
    rgpu, cam, inputs = ref
    params = dict(scenes.ALL_MATERIALS_CAMERA)
    ox, oy, oz = params["origin"]
    cam2 = hb.camera_new(**{**params, "origin": (ox + 0.05, oy, oz)})
    for w, h in FRAMES:
        ins = {k: inputs(w, h)[k] for k in ("color", *GUIDES)}
        run = DeviceRunner(torch, hb, rgpu, w, h)
        for frame, (camera, with_motion) in enumerate(((cam, True), (cam2, False), (cam, True))):
            want, want_motion, _, _ = run.step(ins, camera)
            got = gpu.denoise_temporal(ins["color"], camera, ins["albedo"], ins["normal"], ins["depth"], motion=with_motion)
            if with_motion:
                got, motion = got
                assert_same_bits(motion, want_motion, f"temporal {w}x{h} frame {frame}: motion", nan_equal=True)
            assert_same_bits(got, want, f"temporal {w}x{h} frame {frame}", nan_equal=True)


def host_display(hb, gpu, img, opts, with_histogram):
    """rt_display with the histogram asked for or not (the binding always asks); returns (pixels, histogram or None, state bytes)"""
    h, w = img.shape[:2]
    out = np.zeros((h, w, 3 if opts.pixel_format == abi.RT_PIXEL_RGB8 else 4), np.uint8)
    hist = np.zeros(abi.DISPLAY_HISTOGRAM_BINS, np.uint32) if with_histogram else None
    state = abi.DisplayState()
    rc = hb.lib().rt_display(gpu._h, img.ctypes.data_as(C.POINTER(C.c_float)), C.byref(opts), out.ctypes.data_as(C.c_void_p), C.byref(state),
                             hist.ctypes.data_as(C.POINTER(C.c_uint32)) if with_histogram else None)
    assert rc == 0, rc
    return out, hist, bytes(state)


def test_display_state_across_growth(hb, gpu, ref):
    """two frames per size with a slow adaptation, so that the second depends on the state of the first.  At 13 x 11 the second
    frame is RGBA8 after RGB8: a larger output at the same frame size, so the buffer grows and the state must come along.  A new
    frame size starts from a zero state."""
    import torch
    rgpu, _, _ = ref
    for w, h in FRAMES:
        frames = [np.ascontiguousarray(hdr_frame(w, h, seed=w + k, plant=False) * F32(1 + 3 * k)) for k in range(2)]
        state = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        for k, (fmt, with_hist) in enumerate(((abi.RT_PIXEL_RGB8, True), (abi.RT_PIXEL_RGBA8, False))):
            run = DeviceDisplay(torch, hb, rgpu, w, h, adaptation=0.25, pixel_format=fmt)
            run.state = state  # the _device sequence carries its state in one tensor
            run.upload(frames[k])
            torch.cuda.synchronize()
            run.launch(use_state=True)
            want_px, want_hist, _ = run.read()
            px, hist, state_bytes = host_display(hb, gpu, frames[k], run.opts, with_hist)
            assert_same_bits(px, want_px, f"display {w}x{h} frame {k}", nan_equal=False)
            if with_hist:
                assert_same_bits(hist, want_hist, f"display {w}x{h} frame {k}: histogram", nan_equal=False)
            assert state_bytes == state.cpu().numpy().tobytes(), f"display {w}x{h} frame {k}: state"
        assert state.cpu().numpy()[1] == 2  # two frames went into this state: it was carried, and started from zero


def test_bloom(hb, gpu, ref):
    import torch
    rgpu, _, _ = ref
    for w, h in FRAMES:
        img = hdr_frame(w, h, seed=w)
        run = DeviceBloom(torch, hb, rgpu, w, h, levels=3)
        assert_same_bits(gpu.bloom(img, levels=3), run(img), f"bloom {w}x{h}", nan_equal=True)
        st = abi.DisplayState(ev=0.75, frames=3, metered=-1.0)
        assert_same_bits(gpu.bloom(img, st, levels=3), run(img, (0.75, 3, -1.0)), f"bloom {w}x{h} with a state", nan_equal=True)


def test_dof(hb, gpu, ref):
    import torch
    rgpu, cam, _ = ref
    kw = dict(focus_distance=4.0, blur_scale=5.0, max_radius=4)
    for w, h in FRAMES:
        img, depth = hdr_frame(w, h, seed=h), depth_plane(w, h, "planted")
        run = DeviceDof(torch, hb, rgpu, w, h, cam, **kw)
        want, want_coc = run(img, depth)
        out, coc = gpu.dof(img, depth, cam, coc=True, **kw)
        assert_same_bits(out, want, f"dof {w}x{h}", nan_equal=True)
        assert_same_bits(coc, want_coc, f"dof {w}x{h}: CoC", nan_equal=True)
        assert_same_bits(gpu.dof(img, depth, cam, **kw), run(img, depth, with_coc=False)[0], f"dof {w}x{h} without CoC", nan_equal=True)


def test_upscale(hb, gpu, ref):
    import torch
    rgpu, cam, inputs = ref
    for (w, h), (W, H) in UPSCALES:
        src = inputs(w, h)
        color, src = src["color"], {k: src[k] for k in GUIDES}
        dst = rgpu.render_aov(cam, abi.default_render_opts(W, H, SPP, method=abi.RT_METHOD_MIS, seed=3), channels=GUIDES)
        for s, d in ((src, dst), ({}, {})):
            run = DeviceUpscale(torch, hb, rgpu, color, s, d, W, H)
            run.launch(with_stage=True)
            want, want_stage = run.read()
            out, stage = gpu.upscale(color, src=s, dst=d or (H, W), stage=True)
            assert_same_bits(out, want, f"upscale {w}x{h} -> {W}x{H} guides {sorted(s)}", nan_equal=True)
            assert_same_bits(stage, want_stage, f"upscale {w}x{h} -> {W}x{H}: stage map", nan_equal=False)
            run = DeviceUpscale(torch, hb, rgpu, color, s, d, W, H)
            run.launch(with_stage=False)
            assert_same_bits(gpu.upscale(color, src=s, dst=d or (H, W)), run.read()[0], f"upscale {w}x{h} -> {W}x{H} without the stage map",
                             nan_equal=True)


def test_noise_tiles(hb, gpu, ref):
    import torch
    rgpu, _, _ = ref
    for w, h in FRAMES:
        rng = np.random.default_rng(w)
        lum, var = rng.uniform(0.0, 2.0, (h, w)).astype(F32), rng.uniform(0.0, 0.1, (h, w)).astype(F32)
        d_tiles = torch.full(((h + 7) // 8, (w + 7) // 8), 7.0, dtype=torch.float32, device="cuda:0")
        d_summary = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        d_lum, d_var = to_dev(torch, lum), to_dev(torch, var)
        torch.cuda.synchronize()
        rgpu.noise_tiles_device(d_lum.data_ptr(), d_var.data_ptr(), w, h, d_tiles.data_ptr(), d_summary.data_ptr())
        torch.cuda.synchronize()
        tiles, summary = gpu.noise_tiles(lum, var)
        assert_same_bits(tiles, d_tiles.cpu().numpy(), f"noise_tiles {w}x{h}", nan_equal=True)
        words = d_summary.cpu().numpy().view(np.uint32)
        assert_same_bits(np.array([summary["max_tile_error"]], F32), words[:1].view(F32), f"noise_tiles {w}x{h}: max", nan_equal=True)
        assert (summary["tiles_above"], summary["n_tiles"]) == (int(words[1]), int(words[2]))


def test_robust_combine(hb, gpu, ref):
    import torch
    rgpu, _, inputs = ref
    shapes = {"out": (3, torch.float32), "mean": (3, torch.float32), "gini": (1, torch.float32), "trimmed": (1, torch.uint8),
              "dropped": (1, torch.uint8)}
    for w, h in FRAMES:
        rng = np.random.default_rng(h)
        sums = rng.uniform(0.0, 4.0, (4, h, w, 3)).astype(F32)
        sums[2, h // 2, w // 2] = 1e6  # a firefly in one chunk
        for channels, albedo in ((abi.ROBUST_CHANNELS, inputs(w, h)["albedo"]), (("out",), None), (("out", "gini", "dropped"), None)):
            bufs = {c: torch.full((h, w, shapes[c][0]) if shapes[c][0] == 3 else (h, w), 7, dtype=shapes[c][1], device="cuda:0") for c in channels}
            d_sums, d_albedo = to_dev(torch, sums), (to_dev(torch, albedo) if albedo is not None else None)
            torch.cuda.synchronize()
            rgpu.robust_combine_device(d_sums.data_ptr(), 4, 2, w, h, {c: t.data_ptr() for c, t in bufs.items()},
                                       d_albedo=d_albedo.data_ptr() if albedo is not None else None)
            torch.cuda.synchronize()
            got = gpu.robust_combine(sums, 2, albedo=albedo, channels=channels)
            assert sorted(got) == sorted(channels)
            for c in channels:
                assert_same_bits(got[c], bufs[c].cpu().numpy(), f"robust_combine {w}x{h} {channels}: {c}", nan_equal=True)


def test_matte_extract(hb, gpu, ref):
    import torch
    rgpu, cam, _ = ref
    for w, h in FRAMES:
        layers = rgpu.render_matte(cam, abi.default_render_opts(w, h, SPP, method=abi.RT_METHOD_MIS, seed=3), layers=3)
        ids, cov = layers["ids"], layers["coverage"]
        present = np.unique(ids)
        for sel in (np.concatenate([present[::2][::-1], present[:1]]), np.array([abi.AOV_NO_ID], np.uint32), np.zeros(0, np.uint32)):
            sel = sel.astype(np.uint32)
            d_out = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda:0")
            d_sel = to_dev(torch, np.sort(sel)) if sel.size else None
            d_ids, d_cov = to_dev(torch, ids), to_dev(torch, cov)
            torch.cuda.synchronize()
            rgpu.matte_extract_device(d_ids.data_ptr(), d_cov.data_ptr(), w, h, 3, d_sel.data_ptr() if sel.size else 0, sel.size, d_out.data_ptr())
            torch.cuda.synchronize()
            assert_same_bits(gpu.matte_extract(ids, cov, sel), d_out.cpu().numpy(), f"matte_extract {w}x{h} of {sel.size} ids", nan_equal=True)


def test_composites_sharing_the_denoise_buffer(hb, gpu, ref):
    """the eight calls interleaved on one scene; each must give what the same call gives as the first call of a fresh scene"""
    rgpu, cam, inputs = ref

    def opts(w, h, split=0):
        o = abi.default_render_opts(w, h, SPP, method=abi.RT_METHOD_MIS, seed=5)
        o.sample_split = split
        return o

    small, up = inputs(7, 5), inputs(13, 11)
    dst = rgpu.render_aov(cam, abi.default_render_opts(13, 9, SPP, method=abi.RT_METHOD_MIS, seed=3), channels=GUIDES)
    focus = float(scenes.ALL_MATERIALS_CAMERA["focus_dist"])
    calls = [
        ("render_denoised 13x11", lambda g: g.render_denoised(cam, opts(13, 11))),
        ("render_upscaled 13x11 -> 45x27", lambda g: g.render_upscaled(cam, opts(45, 27), 13, 11)),
        ("render_denoised_split 7x5", lambda g: g.render_denoised_split(cam, opts(7, 5, split=2))),
        ("render_denoised_robust 45x27", lambda g: g.render_denoised_robust(cam, opts(45, 27, split=2))),
        ("upscale 7x5 -> 13x9", lambda g: g.upscale(small["color"], src={k: small[k] for k in GUIDES}, dst=dst, stage=True)),
        ("denoise 13x11", lambda g: (g.denoise(up),)),
        ("render_dof 13x11", lambda g: (g.render_dof(cam, opts(13, 11), hb.dof_opts_from_camera(cam, 2.0, focus, 13, 11, max_radius=4)),)),
        ("render_denoised 13x11 again", lambda g: g.render_denoised(cam, opts(13, 11))),
    ]
    for what, call in calls:
        first, _ = fresh(hb)
        want = call(first)
        first.close()
        got = call(gpu)
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            if isinstance(b, np.ndarray):
                assert_same_bits(a, b, f"{what}: output {k}", nan_equal=True)
            else:
                assert a == b, f"{what}: output {k} (rays shot) {a} != {b}"
