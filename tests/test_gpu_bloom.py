"""The bloom stage (rt_bloom, rt_bloom_device) on the GPU, every comparison bit for bit against the numpy checker
(tests/bloom_checker.py): synthetic HDR frames with planted NaN / inf / negative / -0 / firefly / at-threshold pixels at sizes that
cross the reduce tiles in both axes, every level count and option edge with the fused tail on and off, a device display state,
the host and the device entry between guard words, in place, a strip past every grid cap, graph capture from the first call with
the state changed between replays, a rendered frame through render -> bloom -> display, and side effects."""
import numpy as np
import pytest

import bloom_checker as B
import display_checker as D
import scenes
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture, load_gpu
from post_runners import SCENES, same_state, state_array, state_tuple

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
SIZES = [(1, 1), (2, 2), (3, 5), (13, 11), (33, 17), (67, 35), (150, 130), (300, 200)]
# csrc/rt_bloom.h: a reduce workgroup makes a 32 x 8 tile, at most 1024 workgroups; 256 pixels per expand / composite workgroup
# and trip, at most 1024 workgroups
TILE_W, TILE_H, MAX_TILES, MAX_BLOCKS = 32, 8, 1024, 1024


def hdr_frame(w, h, seed=0, plant=True):
    """log-normal luminances clipped to 2^-10 .. 2^12 under random hues; NaN, +-inf, negatives, -0, a 1e30 firefly and pixels
    exactly at the default threshold (grey 1: Y is the threshold to the last bit or one below) planted where the frame has room"""
    rng = np.random.default_rng(seed)
    lum = np.exp2(np.clip(rng.normal(0.0, 4.0, (h, w, 1)), -10.0, 12.0))
    img = (rng.uniform(0.2, 1.0, (h, w, 3)) * lum).astype(F32)
    if plant:
        flat = img.reshape(-1, 3)
        n = flat.shape[0]
        odd = [(np.nan, 1.0, 1.0), (np.inf, 2.0, 0.5), (0.5, -np.inf, 3.0), (-4.0, -0.5, 8.0), (-0.0, -0.0, -0.0), (1e30, 5e29, 2e30),
               (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (np.nan, np.nan, np.nan), (0.0, 0.0, 0.0)]
        for k, px in enumerate(odd):
            if n > 2 * k + 1:
                flat[(k * 7919 + n // 3) % n] = px
        flat[n - 1] = odd[0] if n > 1 else flat[n - 1]  # the last pixel of the frame
    return np.ascontiguousarray(img)


@pytest.fixture(scope="module")
def dev_scene(hb):
    gpu, cam_params = load_gpu(hb, SCENES, "all_materials")
    return gpu, hb.camera_new(**cam_params)


class DeviceBloom:
    """rt_bloom_device over guarded torch buffers: frame and output one float off 16-byte alignment, the workspace aligned"""

    def __init__(self, torch, hb, gpu, w, h, **opts):
        self.torch, self.gpu, self.w, self.h = torch, gpu, w, h
        self.opts = hb.bloom_opts(w, h, **opts)
        self.ws_words = hb.bloom_workspace_bytes(self.opts) // 4
        self.frames = GuardedBuffers(torch, {"rgb": ((h, w, 3), np.float32), "out": ((h, w, 3), np.float32)}, off=1)
        self.work = GuardedBuffers(torch, {"ws": ((self.ws_words,), np.uint32)}, off=0)
        self.state = torch.zeros(4, dtype=torch.int32, device="cuda:0")

    def upload(self, img, state=None):
        body = self.torch.from_numpy(np.ascontiguousarray(img, F32).view(np.int32).ravel()).to("cuda:0")
        self.frames.buf["rgb"][5:5 + body.numel()] = body
        if state is not None:
            self.state.copy_(self.torch.from_numpy(state_array(state).view(np.int32)).to("cuda:0"))

    def launch(self, use_state=False, in_place=False, stream=0):
        self.gpu.bloom_device(self.frames.ptr("rgb"), self.opts, self.state.data_ptr() if use_state else 0, self.work.ptr("ws"),
                              self.frames.ptr("rgb" if in_place else "out"), stream=stream)

    def read(self, in_place=False):
        self.torch.cuda.synchronize()
        self.work.read("ws")  # the guard words round the workspace
        if in_place:
            assert self.frames.untouched("out")
        return self.frames.read("rgb" if in_place else "out")

    def __call__(self, img, state=None, in_place=False):
        self.frames.refill()
        self.work.refill()
        self.upload(img, state)
        self.torch.cuda.synchronize()
        self.launch(use_state=state is not None, in_place=in_place)
        return self.read(in_place)


@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_and_levels(hb, O, dev_scene, w, h):
    """levels 1, 2, 6 and 12 with the fused tail off and on: identical bytes, and the checker's"""
    import torch
    gpu, _ = dev_scene
    img = hdr_frame(w, h, seed=w + h)
    for levels in (1, 2, 6, 12):
        ref = B.bloom(O, img, levels=levels)
        outs = []
        for fuse in (0, 1):
            run = DeviceBloom(torch, hb, gpu, w, h, levels=levels, fuse_tail=fuse)
            outs.append(run(img))
            assert_same_bits(outs[-1], ref, f"{w}x{h} levels {levels} fuse_tail {fuse}", nan_equal=True)
        assert_same_bits(outs[0], outs[1], f"{w}x{h} levels {levels}: fuse_tail 0 against 1", nan_equal=True)
    if (w, h) == (150, 130):  # level 0 is tiled (3 x 9 tiles), the tail owns levels 1 .. 5
        assert B.level_sizes(w, h, 6)[0] == (75, 65) and B.tail_from(w, h, 6) == 1
    if (w, h) == (300, 200):  # levels 0 and 1 are tiled (the plain reduce runs next to the tail), the tail owns 2 .. 5
        assert B.tail_from(w, h, 6) == 2
    if w * h > 4:
        assert (ref != img)[np.isfinite(img)].any()  # the stage did something


OPTION_CASES = [dict(threshold=0.0), dict(knee=0.0), dict(knee=1.0), dict(scatter=0.0), dict(scatter=1.0), dict(intensity=0.0),
                dict(exposure_ev=3.0), dict(exposure_ev=-3.0), dict(threshold=0.0, knee=0.0, intensity=1.0, clamp_max=50.0),
                dict(threshold=4.0, knee=0.25, scatter=0.9, intensity=0.3, clamp_max=100.0, exposure_ev=0.7)]


@pytest.mark.parametrize("kw", OPTION_CASES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_options(hb, O, dev_scene, kw):
    import torch
    gpu, _ = dev_scene
    for (w, h), levels in (((67, 35), 6), ((150, 130), 4)):
        img = hdr_frame(w, h, seed=11)
        ref = B.bloom(O, img, levels=levels, **kw)
        for fuse in (0, 1):
            run = DeviceBloom(torch, hb, gpu, w, h, levels=levels, fuse_tail=fuse, **kw)
            assert_same_bits(run(img), ref, f"{w}x{h} {kw} fuse_tail {fuse}", nan_equal=True)
    if kw.get("intensity") == 0.0:
        keep = np.isfinite(img)
        assert np.array_equal(ref[keep], img[keep])


def test_device_state_is_read_on_the_device_and_left_alone(hb, O, dev_scene):
    import torch
    gpu, _ = dev_scene
    w, h = 67, 35
    img = hdr_frame(w, h, seed=5)
    state = (F32(1.25), 7, F32(-3.5))
    run = DeviceBloom(torch, hb, gpu, w, h, exposure_ev=-0.5)
    out = run(img, state)
    ev = F32(1.25) + F32(-0.5)
    assert_same_bits(out, B.bloom(O, img, ev=ev), "state.ev + exposure_ev", nan_equal=True)
    assert not np.array_equal(out, B.bloom(O, img, exposure_ev=-0.5), equal_nan=True)  # the state mattered
    after = run.state.cpu().numpy().view(np.uint32)
    assert same_state(state_tuple(after), state) and after[3] == 0 and np.array_equal(after, state_array(state))
    assert_same_bits(run(img), B.bloom(O, img, exposure_ev=-0.5), "no state", nan_equal=True)


def test_host_and_device_entries(hb, O, dev_scene):
    """13 x 11; the device entry between guard words (DeviceBloom.read checks those of the output and the workspace)"""
    import torch
    gpu, _ = dev_scene
    w, h = 13, 11
    img = hdr_frame(w, h, seed=2)
    for kw in (dict(), dict(levels=12, fuse_tail=0, knee=0.0), dict(levels=3, exposure_ev=1.5)):
        ref = B.bloom(O, img, **kw)
        assert_same_bits(gpu.bloom(img, **kw), ref, f"host {kw}", nan_equal=True)
        assert_same_bits(DeviceBloom(torch, hb, gpu, w, h, **kw)(img), ref, f"device {kw}", nan_equal=True)
    st = abi.DisplayState()
    st.ev, st.frames = 2.0, 3
    assert_same_bits(gpu.bloom(img, state=st, exposure_ev=-0.75), B.bloom(O, img, ev=F32(2.0) + F32(-0.75)), "host state", nan_equal=True)
    assert (st.ev, st.frames) == (2.0, 3)
    big = hdr_frame(150, 130, seed=3)  # the scene's buffers grow, then serve the smaller frame again
    assert_same_bits(gpu.bloom(big), B.bloom(O, big), "host 150x130", nan_equal=True)
    assert_same_bits(gpu.bloom(img), B.bloom(O, img), "host 13x11 again", nan_equal=True)


def test_in_place(hb, O, dev_scene):
    import torch
    gpu, _ = dev_scene
    for (w, h), fuse in (((150, 130), 1), ((33, 17), 0)):
        img = hdr_frame(w, h, seed=8)
        run = DeviceBloom(torch, hb, gpu, w, h, fuse_tail=fuse)
        assert_same_bits(run(img, in_place=True), B.bloom(O, img), f"{w}x{h} d_out == d_rgb", nan_equal=True)


def test_strip_past_every_grid_cap(hb, O, dev_scene):
    """262 146 x 4, two levels, no tail (level 1 alone is 65 537 pixels): bloom_reduce<true> has 4097 tiles and bloom_reduce<false>
    2049 against the cap of 1024, bloom_expand_add 262 146 pixels and bloom_composite 1 048 584 against 1024 x 256 per trip.  The
    output starts as guard words, so a skipped pixel fails."""
    import torch
    gpu, _ = dev_scene
    w, h, levels = 262146, 4, 2
    sizes = B.level_sizes(w, h, levels)
    tiles = [-(-a // TILE_W) * -(-b // TILE_H) for a, b in sizes]
    assert min(tiles) > MAX_TILES and sizes[0][0] * sizes[0][1] > 256 * MAX_BLOCKS and w * h > 256 * MAX_BLOCKS
    assert B.tail_from(w, h, levels) == levels
    img = hdr_frame(w, h, seed=9)
    img[h - 1, w - 1] = (300.0, 200.0, 100.0)
    ref = B.bloom(O, img, levels=levels)
    for fuse in (0, 1):
        run = DeviceBloom(torch, hb, gpu, w, h, levels=levels, fuse_tail=fuse)
        assert_same_bits(run(img), ref, f"strip fuse_tail {fuse}", nan_equal=True)
        del run
    torch.cuda.empty_cache()


def test_graph_capture_of_the_first_call_follows_the_state(hb, O):
    """a scene whose first rt_bloom_device is the captured one; the state's ev is rewritten on the device between the replays"""
    import torch
    gpu, _ = load_gpu(hb, SCENES, "rtweekend1")
    w, h = 150, 130
    img = hdr_frame(w, h, seed=4)
    run = DeviceBloom(torch, hb, gpu, w, h, exposure_ev=0.25)
    run.upload(img, (F32(-1.0), 1, F32(0)))
    g = capture(torch, lambda stream: run.launch(use_state=True, stream=stream))
    assert run.frames.untouched("out")  # captured, not run
    for ev in (F32(-1.0), F32(1.5)):
        run.state[0] = int(np.array([ev], F32).view(np.int32)[0])
        torch.cuda.synchronize()
        g.replay()
        assert_same_bits(run.read(), B.bloom(O, img, ev=ev + F32(0.25)), f"replay at state ev {ev}", nan_equal=True)
    gpu.close()


def test_rendered_frame_through_bloom_and_display(hb, O, dev_scene):
    """24 x 20 of the scene with an emissive sphere and triangle: rt_render_device -> rt_bloom_device -> rt_display_device on one
    stream, the display's state handed to the bloom (zero: ev 0)"""
    import torch
    gpu, cam = dev_scene
    w, h = 24, 20
    opts = abi.default_render_opts(w, h, 8, method=abi.RT_METHOD_MIS, seed=3)
    run = DeviceBloom(torch, hb, gpu, w, h, threshold=0.5)
    run.frames.refill()
    dopts = hb.display_opts(w, h)
    dws = torch.zeros(hb.display_workspace_bytes(dopts), dtype=torch.uint8, device="cuda:0")
    px = torch.zeros(hb.display_output_bytes(dopts), dtype=torch.uint8, device="cuda:0")
    hist = torch.zeros(256, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.render_device(cam, opts, run.frames.ptr("rgb"))
    run.launch(use_state=True)
    gpu.display_device(run.frames.ptr("out"), dopts, run.state.data_ptr(), dws.data_ptr(), px.data_ptr(), hist.data_ptr())
    bloomed = run.read()
    frame = run.frames.read("rgb")
    assert frame.tobytes() == gpu.render(cam, opts)[0].tobytes() and (B.lum32(frame) > 0.5).any()
    ref = B.bloom(O, frame, threshold=0.5)
    assert_same_bits(bloomed, ref, "bloom of the rendered frame", nan_equal=True)
    assert (bloomed != frame).any()
    ref_px, ref_hist, ref_state = D.display(O, bloomed, (F32(0), 0, F32(0)))
    assert np.array_equal(px.cpu().numpy().reshape(h, w, 4), ref_px) and np.array_equal(hist.cpu().numpy().view(np.uint32), ref_hist)
    assert same_state(state_tuple(run.state.cpu().numpy().view(np.uint32)), ref_state)


def test_no_side_effects(hb, O, dev_scene):
    import torch
    gpu, cam = dev_scene

    def between(opts, image):
        out = gpu.bloom(image)
        assert_same_bits(out, B.bloom(O, image), "bloom between two renders", nan_equal=True)
        DeviceBloom(torch, hb, gpu, image.shape[1], image.shape[0])(image)

    assert_render_unaffected(gpu, cam, between)
