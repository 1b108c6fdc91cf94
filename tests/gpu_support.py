"""What the GPU test files share: the bit comparison, guarded device buffers, graph capture, the render-is-unaffected check and the
scene loaders.  torch is never imported here: the classes and functions that need it take the module as their first argument, so
the CPU suite can import this file (and collect the GPU files) on a machine without a GPU."""
import numpy as np
import pytest

import scenes

abi = scenes.abi
F32 = np.float32
CAMERA_16_9 = float(F32(16.0) / F32(9.0))


def assert_same_bits(got, ref, what, *, nan_equal):
    """dtype, shape and every element equal.  float32 is compared as uint32 words (+0.0 and -0.0 differ); with nan_equal any NaN
    equals any NaN, without it NaNs compare by payload like every other word.  Other dtypes compare by value."""
    a, b = np.asarray(got), np.asarray(ref)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == np.float32:
        same = a.view(np.uint32) == b.view(np.uint32)
        if nan_equal:
            same = same | (np.isnan(a) & np.isnan(b))
    else:
        same = a == b
    if not np.all(same):
        bad = np.argwhere(~same)
        pytest.fail(f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: gpu {a[tuple(bad[0])]!r} checker {b[tuple(bad[0])]!r}")


class GuardedBuffers:
    """One int32 tensor per channel of `spec` (name -> (shape, np.float32 or np.uint32)), filled with `guard`: four guard words,
    `off` more (the body then starts `off` floats past a 16-byte boundary), the body, and at least nine guard words behind it.
    read() fails if any word outside the body no longer holds the guard."""

    def __init__(self, torch, spec, *, off=0, guard=0x5A5A5A5A, device=None):
        assert 0 <= off <= 3 and 0 <= guard < 1 << 31
        self.spec, self.off, self.guard = dict(spec), off, guard
        self.n = {name: int(np.prod(shape)) for name, (shape, _) in self.spec.items()}
        self.buf = {name: torch.full((n + 16,), guard, dtype=torch.int32, device=device or "cuda:0") for name, n in self.n.items()}

    def ptr(self, name):
        return self.buf[name].data_ptr() + 4 * (4 + self.off)

    def ptrs(self, names=None):
        return {name: self.ptr(name) for name in (self.spec if names is None else names)}

    def refill(self):
        for t in self.buf.values():
            t.fill_(self.guard)

    def untouched(self, name):
        return bool((self.buf[name].cpu().numpy().view(np.uint32) == self.guard).all())

    def read(self, name, used=None):
        """the body in the channel's dtype and shape; with `used`, its first `used` words (rows of the channel's trailing shape),
        and the rest of the body must still hold the guard as well"""
        shape, dtype = self.spec[name]
        a = self.buf[name].cpu().numpy().view(np.uint32)
        lo = 4 + self.off
        hi = lo + (self.n[name] if used is None else used)
        assert (a[:lo] == self.guard).all() and (a[hi:] == self.guard).all(), f"{name}: a guard value was overwritten"
        return a[lo:hi].copy().view(dtype).reshape(shape if used is None else (-1,) + tuple(shape[1:]))

    def read_all(self, names=None):
        return {name: self.read(name) for name in (self.spec if names is None else names)}


def capture(torch, enqueue, side=None):
    """enqueue(stream_handle) captured into a graph on a side stream of cuda:0 (a new one, or `side` where the test has already
    run on one); the device is synchronized before and after.  Nothing has run when this returns: the caller asserts that, and
    replays."""
    dev = torch.device("cuda", 0)
    if side is None:
        side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        enqueue(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return g


def assert_render_unaffected(gpu, cam, between):
    """a 96 x 54 frame of 8 MIS passes, `between(opts, image)`, and the same frame again: the kernel count and the launch info
    describe the render after `between` and after the second render, and that one returns the same bytes and ray count"""
    opts = abi.default_render_opts(96, 54, 8, method=abi.RT_METHOD_MIS, seed=2)
    img_a, rays_a = gpu.render(cam, opts)
    n_a = gpu.last_kernel_ms()[1]
    info_a = gpu.last_launch_info()
    between(opts, img_a)
    assert gpu.last_kernel_ms()[1] == n_a and gpu.last_launch_info() == info_a  # still describe the render
    img_b, rays_b = gpu.render(cam, opts)
    assert np.array_equal(img_a, img_b) and img_a.tobytes() == img_b.tobytes() and rays_a == rays_b
    assert gpu.last_kernel_ms()[1] == n_a and gpu.last_launch_info() == info_a


def radiance_device_run(torch, gpu, o, d, streams, off, **kw):
    """rt_radiance_device on guarded buffers `off` floats past a 16-byte boundary, `streams` (u64 per ray, or None) in a device
    array: returns (GuardedBuffers with "rays" and "out", enqueue(stream handle), the streams tensor to keep alive)"""
    n = len(o)
    bufs = GuardedBuffers(torch, {"rays": ((n, 6), np.float32), "out": ((n, 3), np.float32)}, off=off)
    packed = np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=np.float32).view(np.int32).reshape(-1)
    lo = 4 + off
    bufs.buf["rays"][lo:lo + 6 * n] = torch.from_numpy(packed.copy()).to(bufs.buf["rays"].device)
    d_streams = None if streams is None else torch.from_numpy(streams.astype(np.uint64).view(np.int64).copy()).to("cuda:0")

    def enqueue(s):
        gpu.radiance_device(bufs.ptr("rays"), 0 if d_streams is None else d_streams.data_ptr(), n, bufs.ptr("out"), stream=s, **kw)
    return bufs, enqueue, d_streams


def ssml_scene(name):
    ls = scenes.load_ssml(name)
    return ls.scene, ls.camera_params


def load_gpu(hb, table, name, devices=None):
    """(HipScene on device 0 or on `devices`, camera parameters) of entry `name` of a scene table"""
    sc, cam_params = table[name]()
    gpu = hb.HipScene(sc, devices=devices) if devices else hb.HipScene(sc, device=0)
    return gpu, cam_params


def quality_scene():
    """a perfect mirror sphere and a glass sphere over a checker-textured Lambertian floor, lit by the sky and a lamp"""
    sc = scenes.SceneDescription()
    sc.sphere((0, -1000, 0), 1000.0, sc.lambertian(sc.checkered((0.9, 0.9, 0.9), (0.2, 0.3, 0.6)), 0.8))
    sc.sphere((-0.8, 0.6, 0.0), 0.6, sc.reflect(sc.solid((0.95, 0.95, 0.95)), 0.0))
    sc.sphere((0.8, 0.6, 0.0), 0.6, sc.refract(sc.solid((1.0, 1.0, 1.0)), 1.5))
    sc.sphere((0.0, 6.0, 3.0), 1.0, sc.emissive(sc.solid((1.0, 0.9, 0.8)), 8.0))
    sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (32, 16))
    return sc


QUALITY_CAMERA = dict(origin=(0.0, 2.0, 6.0), lookat=(0.0, 0.8, 0.0), vup=(0.0, 1.0, 0.0), fov=40.0, aspect_ratio=CAMERA_16_9,
                      aperture=0.0, focus_dist=10.0)
QUALITY_MIRROR, QUALITY_GLASS = 1, 2  # material indices in quality_scene()
