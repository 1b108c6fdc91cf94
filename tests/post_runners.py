"""What the test files of the denoiser family (rt_denoise, rt_denoise_temporal, rt_display, rt_upscale and the one-call forms) share:
the scene table, the tolerance, synthetic and rendered inputs, and for each stage its device runner over torch buffers and the
check of one run against the stage's checker.  torch is passed in, never imported (see tests/gpu_support.py)."""
import numpy as np

import denoise_checker as K
import display_checker as D
import scenes
import temporal_checker as T
import upscale_checker as U
from gpu_support import ssml_scene

abi = scenes.abi
F32 = np.float32

# The GPU filters in f32 with the device's expf / powf / sqrtf, the checker in float64: every output pixel must satisfy
#   |gpu - ref| / (|ref| + 1e-3 * mean|ref|) <= 1e-4
# A wrong tap, weight or border rule misses this by orders of magnitude.
TOL = 1e-4

SCENES = {
    "rtweekend1": lambda: ssml_scene("rtweekend1"),
    "overshadowed": lambda: ssml_scene("overshadowed"),
    "pyramid": lambda: ssml_scene("pyramid"),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "structured_meshes": lambda: (scenes.structured_meshes(), scenes.STRUCTURED_CAMERA),
}
SCENES.update({f"random_everything_{seed}": (lambda seed=seed: scenes.random_everything(seed)) for seed in range(4)})


def synthetic(h, w, seed=0):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    return dict(color=rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32), albedo=rng.uniform(0, 1, (h, w, 3)).astype(np.float32),
                normal=n, depth=rng.uniform(0.5, 3.0, (h, w)).astype(np.float32),
                variance=rng.uniform(0, 0.2, (h, w)).astype(np.float32))


def display_mse(img, ref):
    f = lambda a: np.clip(a.astype(np.float64), 0.0, 1.0) ** (1 / 2.2)  # noqa: E731
    return float(((f(img) - f(ref)) ** 2).mean())


# ---- rt_denoise ----
def rendered_inputs(gpu, cam, w, h, spp=8, seed=3, method=abi.RT_METHOD_MIS):
    """color (rt_render of spp passes), the AOVs of the same passes, and the two-halves variance of passes [0, spp/2), [spp/2, spp)"""
    opts = abi.default_render_opts(w, h, spp, method=method, seed=seed)
    color, _ = gpu.render(cam, opts)
    aov = gpu.render_aov(cam, opts, channels=("albedo", "normal", "depth"))
    halves = []
    for begin in (0, spp // 2):
        o = abi.default_render_opts(w, h, spp // 2, method=method, seed=seed)
        o.sample_begin = begin
        halves.append(gpu.render(cam, o)[0])
    return dict(color=color, variance=K.halves_variance(halves[0], halves[1], aov["albedo"]), **aov)


def check_against_checker(gpu_out, inputs, what, **opts):
    ref = K.denoise(inputs["color"], inputs.get("albedo"), inputs.get("normal"), inputs.get("depth"), inputs.get("variance"), **opts)
    assert gpu_out.dtype == np.float32 and gpu_out.shape == ref.shape
    err = K.relative_error(gpu_out, ref)
    assert err <= TOL, f"{what}: relative error {err:.3e}"
    return ref


def device_run(torch, hb, gpu, inputs, opts, stream):
    """rt_denoise_device on `stream` over torch copies of `inputs`; returns the output as numpy"""
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inputs.items()}
    ws = torch.empty(hb.denoise_workspace_bytes(opts), dtype=torch.uint8, device=dev)
    out = torch.full(inputs["color"].shape, 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    gpu.denoise_device({k: v.data_ptr() for k, v in t.items()}, ws.data_ptr(), out.data_ptr(), opts, stream=stream)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


# ---- rt_denoise_temporal ----
def bits_equal(a, b):
    """same bits, NaN == NaN whatever its payload"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


class DeviceRunner:
    """rt_denoise_temporal_device over torch buffers, two histories ping-ponged"""

    def __init__(self, torch, hb, gpu, w, h, **opts):
        self.torch, self.hb, self.gpu, self.w, self.h = torch, hb, gpu, w, h
        self.dev = torch.device("cuda", 0)
        self.opts = hb.temporal_opts(w, h, **opts)
        hb_ = hb.temporal_history_bytes(self.opts)
        self.hist = [torch.full((hb_ // 4,), 7.0, dtype=torch.float32, device=self.dev) for _ in range(2)]
        self.ws = torch.empty(hb.temporal_workspace_bytes(self.opts), dtype=torch.uint8, device=self.dev)
        self.out = torch.zeros(h * w * 3, dtype=torch.float32, device=self.dev)
        self.motion = torch.zeros(h * w * 2, dtype=torch.float32, device=self.dev)
        self.cur, self.prev = -1, None

    def upload(self, inputs):
        self.t = {k: self.torch.from_numpy(np.ascontiguousarray(v)).to(self.dev) for k, v in inputs.items()}

    def launch(self, cam, stream=0):
        nxt = 1 if self.cur == 0 else 0
        h_in = self.hist[self.cur].data_ptr() if self.cur >= 0 else 0
        self.gpu.denoise_temporal_device({k: v.data_ptr() for k, v in self.t.items()}, cam, self.prev, h_in,
                                         self.hist[nxt].data_ptr(), self.ws.data_ptr(), self.out.data_ptr(), self.opts,
                                         d_motion=self.motion.data_ptr(), stream=stream)
        self.cur, self.prev = nxt, cam

    def step(self, inputs, cam):
        """one frame; returns (out, motion, history written, history read or None) as numpy"""
        h_in = self.history(self.cur) if self.cur >= 0 else None
        self.upload(inputs)
        self.torch.cuda.synchronize(self.dev)
        self.launch(cam)
        self.torch.cuda.synchronize(self.dev)
        return (self.out.cpu().numpy().reshape(self.h, self.w, 3), self.motion.cpu().numpy().reshape(self.h, self.w, 2),
                self.history(self.cur), h_in)

    def history(self, i):
        return T.history_array(self.hist[i].cpu().numpy(), self.h, self.w)


def check_step(inputs, cam, prev, h_in, out, motion, h_out, what, iterations=5, normal=True, **opts):
    """`opts`: the temporal options and sigmas the GPU ran with, for the checker (the defaults when none are given)"""
    st = T.step(inputs["color"], inputs["depth"], cam, prev, h_in, albedo=inputs.get("albedo"),
                normal=inputs.get("normal") if normal else None, **opts)
    assert bits_equal(motion, st["motion"]), f"{what}: motion"
    assert bits_equal(h_out[0, ..., 3], st["n"]), f"{what}: n"
    assert bits_equal(h_out[2, ..., 0], st["m1"]) and bits_equal(h_out[2, ..., 1], st["m2"]), f"{what}: moments"
    assert bits_equal(h_out[1], st["history"][1]), f"{what}: n^ and z"
    assert not h_out[2, ..., 2:].any(), what
    e1, ref = T.filtered(st, inputs["color"], normal, iterations=iterations, **{k: v for k, v in opts.items() if k.startswith("sigma_")})
    ok = st["valid"]
    assert np.array_equal(out[~ok], inputs["color"][~ok], equal_nan=True), f"{what}: invalid pixels pass through"
    err_e1, err_out = K.relative_error(h_out[0][ok][:, :3], e1[ok]), K.relative_error(out[ok], ref[ok])
    assert err_e1 <= TOL and err_out <= TOL, f"{what}: e_1 {err_e1:.3e} out {err_out:.3e}"
    return st


# ---- rt_display ----
def state_array(st):
    """(ev, frames, metered) -> the 16 bytes of an rt_display_state"""
    a = np.zeros(4, np.uint32)
    a[0] = np.array([st[0]], F32).view(np.uint32)[0]
    a[1] = st[1]
    a[2] = np.array([st[2]], F32).view(np.uint32)[0]
    return a


def state_tuple(a):
    a = np.asarray(a, np.uint32)
    return (a[0:1].view(F32)[0], int(a[1]), a[2:3].view(F32)[0])


def same_state(a, b):
    return (np.array([a[0]], F32).view(np.uint32)[0] == np.array([b[0]], F32).view(np.uint32)[0] and a[1] == b[1]
            and ((np.isnan(a[2]) and np.isnan(b[2])) or np.array([a[2]], F32).view(np.uint32)[0] == np.array([b[2]], F32).view(np.uint32)[0]))


class DeviceDisplay:
    """rt_display_device over torch buffers; in_off / out_off shift the input (floats) and the output (bytes) off 16-byte alignment"""

    def __init__(self, torch, hb, gpu, w, h, in_off=0, out_off=0, **opts):
        self.torch, self.gpu, self.w, self.h, self.in_off, self.out_off = torch, gpu, w, h, in_off, out_off
        self.dev = torch.device("cuda", 0)
        self.opts = hb.display_opts(w, h, **opts)
        self.nbytes = hb.display_output_bytes(self.opts)
        self.src = torch.zeros(w * h * 3 + 4, dtype=torch.float32, device=self.dev)
        self.ws = torch.full((hb.display_workspace_bytes(self.opts),), 0xA5, dtype=torch.uint8, device=self.dev)
        self.out = torch.full((self.nbytes + 16,), 0x5A, dtype=torch.uint8, device=self.dev)
        self.hist = torch.zeros(256, dtype=torch.int32, device=self.dev)
        self.state = torch.zeros(4, dtype=torch.int32, device=self.dev)

    def upload(self, img, state=None):
        n = img.size
        self.src[self.in_off:self.in_off + n] = self.torch.from_numpy(np.ascontiguousarray(img, F32).ravel()).to(self.dev)
        if state is not None:
            self.state.copy_(self.torch.from_numpy(state_array(state).view(np.int32)).to(self.dev))

    def launch(self, use_state=True, stream=0):
        self.gpu.display_device(self.src.data_ptr() + 4 * self.in_off, self.opts, self.state.data_ptr() if use_state else 0,
                                self.ws.data_ptr(), self.out.data_ptr() + self.out_off, self.hist.data_ptr(), stream=stream)

    def read(self):
        self.torch.cuda.synchronize(self.dev)
        o = self.out.cpu().numpy()
        assert (o[:self.out_off] == 0x5A).all() and (o[self.out_off + self.nbytes:] == 0x5A).all(), "wrote outside the output"
        px = o[self.out_off:self.out_off + self.nbytes].reshape(self.h, self.w, -1)
        return px, self.hist.cpu().numpy().view(np.uint32), state_tuple(self.state.cpu().numpy().view(np.uint32))

    def __call__(self, img, state=None):
        self.upload(img, state)
        self.torch.cuda.synchronize(self.dev)
        self.launch(use_state=state is not None)
        return self.read()


def check_display(O, run, img, state, what, **opts):
    px, hist, st = run(img, state)
    ref_px, ref_hist, ref_st = D.display(O, img, state, **opts)
    assert np.array_equal(hist, ref_hist), f"{what}: histogram"
    assert px.shape == ref_px.shape and np.array_equal(px, ref_px), \
        f"{what}: {int((px != ref_px).sum())} bytes differ"
    if state is not None:
        assert same_state(st, ref_st), f"{what}: state {st} vs {ref_st}"
    return px, ref_st


# ---- rt_upscale ----
GUIDES = ("albedo", "normal", "depth")
STAGES_SEEN = set()  # the union of the stage maps of every check_upscale of this process: tests/test_gpu_upscale.py asserts on it


def library_inputs(gpu, cam, w, h, W, H, spp=8, seed=3):
    """the filtered source frame (rt_render_denoised at w x h) and the rt_render_aov guides at both sizes"""
    so = abi.default_render_opts(w, h, spp, method=abi.RT_METHOD_MIS, seed=seed)
    clean, _, _ = gpu.render_denoised(cam, so)
    src = gpu.render_aov(cam, so, channels=GUIDES)
    dst = gpu.render_aov(cam, abi.default_render_opts(W, H, spp, method=abi.RT_METHOD_MIS, seed=seed), channels=GUIDES)
    return clean, src, dst


def check_upscale(O, gpu, color, src, dst, W, H, what, **opts):
    """host entry against the checker: frame and stage map, bit for bit"""
    out, stage = gpu.upscale(color, src=src, dst=dst if dst else (H, W), stage=True, **opts)
    ref, ref_stage = U.upscale(O, color, W, H, src=src, dst=dst, **opts)
    STAGES_SEEN.update(int(v) for v in np.unique(stage))
    assert np.array_equal(stage, ref_stage), f"{what}: {int((stage != ref_stage).sum())} stage values differ"
    same = out.view(np.uint32) == ref.view(np.uint32)
    assert same.all(), f"{what}: {int((~same).sum())} floats differ, max |d| {np.nanmax(np.abs(out - ref)):.3e}"
    return out, stage


class DeviceUpscale:
    """rt_upscale_device over torch buffers; `off` shifts every float buffer by that many floats and the stage map by as many bytes"""

    def __init__(self, torch, hb, gpu, color, src, dst, W, H, off=0, **opts):
        self.torch, self.gpu, self.W, self.H, self.off = torch, gpu, W, H, off
        self.dev = torch.device("cuda", 0)
        h, w = color.shape[:2]
        self.opts = hb.upscale_opts(w, h, W, H, **opts)
        arrays = {"color": color, **{"src_" + k: v for k, v in src.items()}, **{"dst_" + k: v for k, v in dst.items()}}
        self.bufs = {}
        for k, a in arrays.items():
            t = torch.zeros(a.size + off, dtype=torch.float32, device=self.dev)
            t[off:] = torch.from_numpy(np.ascontiguousarray(a, F32).ravel()).to(self.dev)
            self.bufs[k] = t
        self.out = torch.full((W * H * 3 + off + 4,), 7.0, dtype=torch.float32, device=self.dev)
        self.stage = torch.full((W * H + off + 16,), 0x5A, dtype=torch.uint8, device=self.dev)

    def launch(self, stream=0, with_stage=True):
        self.gpu.upscale_device({k: t.data_ptr() + 4 * self.off for k, t in self.bufs.items()}, self.out.data_ptr() + 4 * self.off,
                                self.opts, self.stage.data_ptr() + self.off if with_stage else 0, stream=stream)

    def read(self):
        self.torch.cuda.synchronize(self.dev)
        o, s = self.out.cpu().numpy(), self.stage.cpu().numpy()
        n = self.W * self.H
        assert (o[:self.off] == 7.0).all() and (o[self.off + 3 * n:] == 7.0).all(), "wrote outside the output"
        assert (s[:self.off] == 0x5A).all() and (s[self.off + n:] == 0x5A).all(), "wrote outside the stage map"
        return o[self.off:self.off + 3 * n].reshape(self.H, self.W, 3).copy(), s[self.off:self.off + n].reshape(self.H, self.W).copy()
