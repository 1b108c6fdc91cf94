"""The depth-of-field stage (rt_dof, rt_dof_device, rt_render_dof) on the GPU, every comparison bit for bit against the numpy checker
(tests/dof_checker.py), frame AND signed circle-of-confusion plane: synthetic HDR frames with planted NaN / inf / negative / -0 /
firefly pixels over synthetic depth (a ramp through the focus distance, a step edge, planted 0 / negative / NaN / +inf depths and
one exactly at the focus distance) at sizes that cross the gather's tile and its halo in both axes, every radius cap, blur scales
that switch the stage off, leave every radius at its floor and push every radius to the cap, with and without a camera, the host
and the device entry between guard words, a strip past both grid caps, graph capture from the first call with the depth changed
between replays, a rendered frame through rt_render_dof, and side effects."""
import numpy as np
import pytest

import dof_checker as K
import scenes
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture, load_gpu
from post_runners import SCENES
from test_gpu_bloom import hdr_frame

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
SIZES = [(1, 1), (2, 2), (3, 5), (13, 11), (33, 17), (67, 35)]
# csrc/rt_dof.h: a gather workgroup makes a 32 x 8 tile, at most 2048 workgroups; 256 pixels per circle-of-confusion workgroup and
# trip, at most 1024 workgroups
TILE_W, TILE_H, MAX_TILES, MAX_BLOCKS = 32, 8, 2048, 1024
FOCUS = 4.0


def depth_plane(w, h, kind, seed=0):
    """ramp: 1 .. 16 across the frame, through FOCUS, wobbling down the rows; step: a near half (1.5) against a far half (40);
    planted: the ramp with 0 (sky), a negative, NaN, +inf, a subnormal and FOCUS itself planted where the frame has room"""
    x = np.linspace(0.0, 1.0, w, dtype=np.float64)[None, :]
    y = np.linspace(0.0, 1.0, h, dtype=np.float64)[:, None]
    if kind == "step":
        z = np.where(x + 0.3 * y < 0.6, 1.5, 40.0) * np.ones((h, w))
    else:
        z = np.exp2(4.0 * x) * (1.0 + 0.1 * np.sin(7.0 * y))
    z = z.astype(F32)
    if kind == "planted":
        flat = z.reshape(-1)
        n = flat.shape[0]
        for k, v in enumerate((0.0, -2.0, np.nan, np.inf, 1e-45, FOCUS, FOCUS, 0.0)):
            if n > 2 * k + 1:
                flat[(k * 7907 + n // 5) % n] = v
        rng = np.random.default_rng(seed)
        flat[rng.integers(0, n, max(1, n // 9))] = 0.0  # patches of sky
    return np.ascontiguousarray(z)


@pytest.fixture(scope="module")
def dev_scene(hb):
    gpu, cam_params = load_gpu(hb, SCENES, "all_materials")
    return gpu, hb.camera_new(**cam_params)


class DeviceDof:
    """rt_dof_device over guarded torch buffers: frame, depth, output and CoC plane one float off 16-byte alignment, the workspace
    aligned"""

    def __init__(self, torch, hb, gpu, w, h, camera=None, **opts):
        self.torch, self.gpu, self.w, self.h, self.camera = torch, gpu, w, h, camera
        self.opts = hb.dof_opts(w, h, **opts)
        self.ws_words = hb.dof_workspace_bytes(self.opts) // 4
        self.frames = GuardedBuffers(torch, {"rgb": ((h, w, 3), np.float32), "out": ((h, w, 3), np.float32),
                                             "depth": ((h, w), np.float32), "coc": ((h, w), np.float32)}, off=1)
        self.work = GuardedBuffers(torch, {"ws": ((self.ws_words,), np.uint32)}, off=0)

    def put(self, name, a):
        body = self.torch.from_numpy(np.ascontiguousarray(a, F32).view(np.int32).ravel()).to("cuda:0")
        self.frames.buf[name][5:5 + body.numel()] = body

    def launch(self, with_coc=True, stream=0):
        self.gpu.dof_device(self.frames.ptr("rgb"), self.frames.ptr("depth"), self.camera, self.opts, self.work.ptr("ws"),
                            self.frames.ptr("out"), self.frames.ptr("coc") if with_coc else 0, stream=stream)

    def read(self, with_coc=True):
        """(out, coc); every guard word round the five buffers is checked, and the inputs must be what was uploaded"""
        self.torch.cuda.synchronize()
        self.work.read("ws")
        if not with_coc:
            assert self.frames.untouched("coc")
        return self.frames.read("out"), (self.frames.read("coc") if with_coc else None)

    def __call__(self, img, depth, with_coc=True):
        self.frames.refill()
        self.work.refill()
        self.put("rgb", img)
        self.put("depth", depth)
        self.torch.cuda.synchronize()
        self.launch(with_coc)
        out, coc = self.read(with_coc)
        assert_same_bits(self.frames.read("rgb"), np.ascontiguousarray(img, F32), "the frame is read only", nan_equal=False)
        assert_same_bits(self.frames.read("depth"), np.ascontiguousarray(depth, F32), "the depth is read only", nan_equal=False)
        return out, coc


def check(torch, hb, gpu, img, depth, what, camera=None, **opts):
    h, w = depth.shape
    ref, ref_coc = K.dof(img, depth, camera, coc=True, **opts)
    out, coc = DeviceDof(torch, hb, gpu, w, h, camera, **opts)(img, depth)
    assert_same_bits(coc, ref_coc, f"{what}: CoC plane", nan_equal=False)
    assert_same_bits(out, ref, what, nan_equal=True)
    return ref, ref_coc


@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_and_radius_caps(hb, dev_scene, w, h):
    """max_radius 1, 2, 8, 16 over the planted ramp, the distance along the ray (no camera) and along the axis (camera)"""
    import torch
    gpu, cam = dev_scene
    img = hdr_frame(w, h, seed=w + h)
    depth = depth_plane(w, h, "planted", seed=w)
    for R in (1, 2, 8, 16):
        ref, coc = check(torch, hb, gpu, img, depth, f"{w}x{h} R {R} radial", focus_distance=FOCUS, blur_scale=6.0, max_radius=R,
                         planar_depth=0)
        assert np.abs(coc).max() <= R and np.abs(coc).min() >= 0.5
        if w >= 2 and h >= 2:
            check(torch, hb, gpu, img, depth, f"{w}x{h} R {R} planar", camera=cam, focus_distance=FOCUS, blur_scale=6.0, max_radius=R)
            check(torch, hb, gpu, img, depth, f"{w}x{h} R {R} camera given, radial", camera=cam, focus_distance=FOCUS, blur_scale=6.0,
                  max_radius=R, planar_depth=0)
    if w * h > 100:
        assert (coc < 0).any() and (coc > 0).any()  # both sides of the focus plane
        finite = np.isfinite(img).all(axis=2)
        assert (ref[finite] != img[finite]).any()  # the stage did something


@pytest.mark.parametrize("kind", ["ramp", "step", "planted"])
def test_depth_shapes(hb, dev_scene, kind):
    import torch
    gpu, cam = dev_scene
    for (w, h), R in (((67, 35), 8), ((33, 17), 16)):
        img = hdr_frame(w, h, seed=3)
        depth = depth_plane(w, h, kind)
        for scale in (1.5, 12.0):
            check(torch, hb, gpu, img, depth, f"{kind} {w}x{h} R {R} scale {scale}", camera=cam, focus_distance=FOCUS, blur_scale=scale,
                  max_radius=R)
    if kind == "step":  # the near side's blur spreads over the edge, the far side's stops at it: the two sides differ
        _, coc = K.dof(img, depth, cam, coc=True, focus_distance=FOCUS, blur_scale=12.0, max_radius=16)
        assert (coc < 0).any() and (coc > 0).any()


def test_blur_scale_off_floor_and_cap(hb, dev_scene):
    import torch
    gpu, cam = dev_scene
    w, h = 67, 35
    img = hdr_frame(w, h, seed=6)
    depth = depth_plane(w, h, "planted")
    for R in (1, 8, 16):
        ref, coc = check(torch, hb, gpu, img, depth, f"off, R {R}", camera=cam, focus_distance=FOCUS, blur_scale=0.0, max_radius=R)
        assert ref.tobytes() == img.tobytes() and (np.abs(coc) == F32(0.5)).all()  # the input's bytes back, -0 and NaN included
        ref, coc = check(torch, hb, gpu, img, depth, f"floor, R {R}", focus_distance=FOCUS, blur_scale=1e-3, max_radius=R, planar_depth=0)
        real = np.isfinite(depth) & (depth > 1e-3)
        assert (np.abs(coc[real]) == F32(0.5)).all()  # (the subnormal depth and the pixels at infinity have k >= 1)
        ref, coc = check(torch, hb, gpu, img, depth, f"cap, R {R}", focus_distance=FOCUS, blur_scale=1e6, max_radius=R, planar_depth=0)
        assert (np.abs(coc[depth != F32(FOCUS)]) == F32(R)).all() and (coc[depth == F32(FOCUS)] == F32(0.5)).all()


def test_a_frame_narrower_than_the_halo(hb, dev_scene):
    import torch
    gpu, cam = dev_scene
    for w, h in ((9, 50), (50, 3)):
        img = hdr_frame(w, h, seed=7)
        check(torch, hb, gpu, img, depth_plane(w, h, "planted"), f"{w}x{h} R 16", camera=cam, focus_distance=FOCUS, blur_scale=20.0,
              max_radius=16)


def test_host_and_device_entries(hb, dev_scene):
    """13 x 11; the device entry between guard words, with and without the CoC plane"""
    import torch
    gpu, cam = dev_scene
    w, h = 13, 11
    img = hdr_frame(w, h, seed=2)
    depth = depth_plane(w, h, "planted")
    for camera, kw in ((cam, dict(focus_distance=FOCUS, blur_scale=5.0)), (None, dict(blur_scale=3.0, max_radius=16, planar_depth=0)),
                       (cam, dict(focus_distance=2.0, blur_scale=9.0, max_radius=2, planar_depth=0))):
        ref, ref_coc = K.dof(img, depth, camera, coc=True, **kw)
        out, coc = gpu.dof(img, depth, camera, coc=True, **kw)
        assert_same_bits(out, ref, f"host {kw}", nan_equal=True)
        assert_same_bits(coc, ref_coc, f"host CoC {kw}", nan_equal=False)
        assert_same_bits(gpu.dof(img, depth, camera, **kw), ref, f"host without CoC {kw}", nan_equal=True)
        run = DeviceDof(torch, hb, gpu, w, h, camera, **kw)
        assert_same_bits(run(img, depth, with_coc=False)[0], ref, f"device without CoC {kw}", nan_equal=True)
        assert_same_bits(run(img, depth)[0], ref, f"device {kw}", nan_equal=True)
    big = hdr_frame(150, 130, seed=3)  # the scene's buffers grow, then serve the smaller frame again
    kw = dict(focus_distance=FOCUS, blur_scale=4.0, max_radius=4)
    assert_same_bits(gpu.dof(big, depth_plane(150, 130, "ramp"), cam, **kw), K.dof(big, depth_plane(150, 130, "ramp"), cam, **kw),
                     "host 150x130", nan_equal=True)
    assert_same_bits(gpu.dof(img, depth, cam, **kw), K.dof(img, depth, cam, **kw), "host 13x11 again", nan_equal=True)


def test_strip_past_both_grid_caps(hb, dev_scene):
    """65 570 x 4 at max_radius 1: dof_gather_kernel has 2050 tiles against the cap of 2048, dof_coc_kernel 262 280 pixels against
    1024 x 256 per trip.  The output starts as guard words, so a skipped pixel fails."""
    import torch
    gpu, cam = dev_scene
    w, h = 65570, 4
    assert -(-w // TILE_W) * -(-h // TILE_H) > MAX_TILES and w * h > 256 * MAX_BLOCKS
    img = hdr_frame(w, h, seed=9)
    img[h - 1, w - 1] = (300.0, 200.0, 100.0)
    depth = depth_plane(w, h, "planted")
    depth[h - 1, w - 2:] = 1.0
    check(torch, hb, gpu, img, depth, "strip", camera=cam, focus_distance=FOCUS, blur_scale=2.0, max_radius=1)
    torch.cuda.empty_cache()


def test_graph_capture_of_the_first_call_follows_the_depth(hb):
    """a scene whose first rt_dof_device is the captured one; the depth plane is rewritten on the device between the replays"""
    import torch
    gpu, cam_params = load_gpu(hb, SCENES, "rtweekend1")
    cam = hb.camera_new(**cam_params)
    w, h = 67, 35
    img = hdr_frame(w, h, seed=4)
    kw = dict(focus_distance=FOCUS, blur_scale=7.0, max_radius=8)
    run = DeviceDof(torch, hb, gpu, w, h, cam, **kw)
    run.put("rgb", img)
    run.put("depth", depth_plane(w, h, "ramp"))
    g = capture(torch, lambda stream: run.launch(stream=stream))
    assert run.frames.untouched("out") and run.frames.untouched("coc")  # captured, not run
    for kind in ("step", "planted"):
        depth = depth_plane(w, h, kind)
        run.put("depth", depth)
        torch.cuda.synchronize()
        g.replay()
        out, coc = run.read()
        ref, ref_coc = K.dof(img, depth, cam, coc=True, **kw)
        assert_same_bits(out, ref, f"replay over the {kind} depth", nan_equal=True)
        assert_same_bits(coc, ref_coc, f"replay over the {kind} depth: CoC", nan_equal=False)
    gpu.close()


def test_render_dof_is_its_parts(hb, dev_scene):
    """24 x 20 of the scene with every material: rt_render_dof against rt_render + the depth of rt_render_aov + the checker, with
    the options rt_dof_opts_from_camera makes of an aperture (the sizes in them are zeroed: the render's are used)"""
    gpu, cam = dev_scene
    w, h = 24, 20
    opts = abi.default_render_opts(w, h, 8, method=abi.RT_METHOD_MIS, seed=3)
    focus = float(scenes.ALL_MATERIALS_CAMERA["focus_dist"])
    dopts = hb.dof_opts_from_camera(cam, 2.0, focus, w, h, max_radius=4)
    assert dopts.blur_scale > 1
    dopts.width = dopts.height = 0
    frame, _ = gpu.render(cam, opts)
    depth = gpu.render_aov(cam, opts, channels=("depth",))["depth"]
    assert (depth > 0).any()
    kw = dict(focus_distance=dopts.focus_distance, blur_scale=dopts.blur_scale, max_radius=4, planar_depth=1)
    ref, coc = K.dof(frame, depth, cam, coc=True, **kw)
    assert np.abs(coc).max() > 1.0  # something is out of focus
    assert_same_bits(gpu.render_dof(cam, opts, dopts), ref, "rt_render_dof", nan_equal=True)
    assert (ref != frame).any()
    assert_same_bits(gpu.dof(frame, depth, cam, **kw), ref, "rt_dof of the parts", nan_equal=True)


def test_no_side_effects(hb, dev_scene):
    import torch
    gpu, cam = dev_scene

    def between(opts, image):
        h, w = image.shape[:2]
        depth = depth_plane(w, h, "ramp")
        kw = dict(focus_distance=FOCUS, blur_scale=3.0, max_radius=2)
        assert_same_bits(gpu.dof(image, depth, cam, **kw), K.dof(image, depth, cam, **kw), "dof between two renders", nan_equal=True)
        DeviceDof(torch, hb, gpu, w, h, cam, **kw)(image, depth)

    assert_render_unaffected(gpu, cam, between)
