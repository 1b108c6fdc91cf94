"""Firefly-robust frames on the GPU against the numpy checker (tests/robust_checker.py): rt_render_robust[_device],
rt_robust_combine[_device] and rt_render_denoised_robust.  Every comparison is bit for bit (NaN == NaN).  The passes of a scene
come from the CPU oracle once per (scene, frame, method, window) and are shared."""
import functools
import itertools

import numpy as np
import pytest

import aov_checker as K
import noise_checker as N
import robust_checker as R
import scenes
from gpu_support import GuardedBuffers, assert_same_bits, capture, ssml_scene

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
SEED = 3
WHOLE, RAGGED = (24, 20), (13, 11)  # whole and half tiles; ragged on both axes
MIS, NAIVE = abi.RT_METHOD_MIS, abi.RT_METHOD_NAIVE
MODES = (dict(mode=R.TRIM, trim=1), dict(mode=R.MEDIAN), dict(mode=R.GINI))
PLANES = ("out", "mean", "gini", "trimmed", "dropped")
OPTIONAL = PLANES[1:]


SCENES = {  # the set of tests/test_gpu_ao.py: spheres, triangles, lights, textured sky, all materials
    "emit_scene": lambda: (K.emit_scene(), K.EMIT_CAMERA),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "spheres500": lambda: (scenes.random_spheres(500), scenes.ALL_MATERIALS_CAMERA),
    "pyramid": lambda: ssml_scene("pyramid"),
    "rtweekend1": lambda: ssml_scene("rtweekend1"),
    "overshadowed": lambda: ssml_scene("overshadowed"),
    "mesh2000_wide": lambda: (scenes.random_triangle_mesh(2000, edge=2.0), scenes.MESH_CAMERA),
    "mesh20000": lambda: (scenes.random_triangle_mesh(20000, edge=1.0), scenes.MESH_CAMERA),
}


@functools.lru_cache(maxsize=None)
def _built(name):
    import oracle as O
    O.build()
    sc, cam_params = SCENES[name]()
    return sc, cam_params, O.Scene(sc), O.camera_new(**cam_params)


def _opts(size, spp, split, method=MIS, seed=SEED, sample_begin=0):
    o = abi.default_render_opts(size[0], size[1], spp, method=method, seed=seed)
    o.sample_begin, o.sample_split = sample_begin, split
    return o


@functools.lru_cache(maxsize=None)
def _passes(name, size, method, seed, sample_begin, n):
    _, _, cpu, cam = _built(name)
    p = N.passes(cpu, cam, _opts(size, 1, 1, method, seed), n, sample_begin)
    p.setflags(write=False)
    return p


def _expected(name, size, method, spp, split, albedo=None, seed=SEED, sample_begin=0, **ropts):
    return R.robust(N.chunk_sums(_passes(name, size, method, seed, sample_begin, spp), split), spp // split, albedo, **ropts)


def _gpu(hb, name):
    sc, cam_params, _, _ = _built(name)
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


def assert_robust(got, ref, what, channels=PLANES):
    for name in channels:
        assert_same_bits(got[name], ref[name], f"{what} {name}", nan_equal=True)


class DeviceRobust(GuardedBuffers):
    """the five outputs in device memory, each with guard values before and after, `off` floats past a 16-byte boundary; the two
    byte planes start one byte further still, and the bytes of their last word behind the frame must keep the guard too"""

    def __init__(self, torch, w, h, off=0):
        self.px, self.h, self.w = w * h, h, w
        words = (self.px + 1 + 3) // 4
        super().__init__(torch, {"out": ((h, w, 3), F32), "mean": ((h, w, 3), F32), "gini": ((h, w), F32),
                                 "trimmed": ((words,), np.uint32), "dropped": ((words,), np.uint32)}, off=off)
        self.rays = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def ptr(self, name):
        return super().ptr(name) + (1 if name in ("trimmed", "dropped") else 0)

    def read(self, name, used=None):
        a = super().read(name, used)
        if name not in ("trimmed", "dropped"):
            return a
        b = a.view(np.uint8)
        assert b[0] == 0x5A and (b[1 + self.px:] == 0x5A).all(), f"{name}: a guard byte was overwritten"
        return b[1:1 + self.px].reshape(self.h, self.w).copy()


# ---- rendered scenes: every scene, three splits, three modes, with and without the albedo ----
@pytest.mark.parametrize("name,method", [(n, MIS) for n in SCENES] + [("all_materials", NAIVE)])
def test_scenes_match_the_checker(hb, name, method):
    gpu, cam = _gpu(hb, name)
    spp = 32
    albedo = gpu.render_aov(cam, _opts(WHOLE, spp, 1, method), channels=("albedo",))["albedo"]
    trimmed = 0
    for split in (4, 8, 16):
        o = _opts(WHOLE, spp, split, method)
        image, rays = gpu.render(cam, o)
        plain = gpu.render_robust(cam, o, mode="trim", trim=0)
        assert plain["out"].tobytes() == image.tobytes() == plain["mean"].tobytes(), f"{name} S={split}: trim 0 is not rt_render"
        for kw in MODES:
            for alb in (None, albedo):
                what = f"{name} method={method} S={split} {kw} albedo={alb is not None}"
                got = gpu.render_robust(cam, o, albedo=alb, **kw)
                assert got["mean"].tobytes() == image.tobytes() and got["rays_shot"] == rays, f"{what}: not the bytes of rt_render"
                assert gpu.last_launch_info()["sample_split"] == split
                ref = _expected(name, WHOLE, method, spp, split, alb, **kw)
                assert_robust(got, ref, what)
                trimmed += int((ref["trimmed"] > 0).sum())
    assert trimmed > 50, "a frame on which nothing is trimmed would test nothing"


@pytest.mark.parametrize("split", [2, 4, 8])
def test_a_ragged_frame_through_the_host_and_the_device_entry(hb, split):
    import torch
    name, spp = "all_materials", 8
    gpu, cam = _gpu(hb, name)
    w, h = RAGGED
    o = _opts(RAGGED, spp, split)
    albedo = gpu.render_aov(cam, o, channels=("albedo",))["albedo"]
    d_albedo = torch.from_numpy(albedo).to("cuda:0")
    image, rays = gpu.render(cam, o)
    for alb, d_alb in ((None, None), (albedo, d_albedo.data_ptr())):
        ref = _expected(name, RAGGED, MIS, spp, split, alb, mode=R.MEDIAN)
        assert ref["mean"].tobytes() == image.tobytes()  # the checker's combine is rt_render's
        assert_robust(gpu.render_robust(cam, o, albedo=alb, mode="median"), ref, f"host S={split} albedo={alb is not None}")
        for off in (0, 1, 3):
            run = DeviceRobust(torch, w, h, off=off)
            torch.cuda.synchronize()
            gpu.render_robust_device(cam, o, run.ptrs(), d_albedo=d_alb, d_rays_ptr=run.rays.data_ptr(), mode="median")
            torch.cuda.synchronize()
            assert_robust(run.read_all(), ref, f"device S={split} albedo={alb is not None} off={off}")
            assert int(run.rays.item()) == rays
    # every subset of the optional planes
    ref = _expected(name, RAGGED, MIS, spp, split, albedo)
    for k in range(len(OPTIONAL) + 1):
        for subset in itertools.combinations(OPTIONAL, k):
            channels = ("out",) + subset
            part = DeviceRobust(torch, w, h, off=1)
            torch.cuda.synchronize()
            gpu.render_robust_device(cam, o, part.ptrs(channels), d_albedo=d_albedo.data_ptr())
            torch.cuda.synchronize()
            assert_robust(part.read_all(channels), ref, f"planes {channels}", channels)
            for name_ in OPTIONAL:
                assert name_ in subset or part.untouched(name_), f"{name_} was written though not asked for"
            host = gpu.render_robust(cam, o, albedo=albedo, channels=subset)
            assert set(host) == set(channels) | {"rays_shot"}
            assert_robust(host, ref, f"host planes {channels}", channels)


def test_sixty_four_chunks_of_one_pass(hb):
    name, spp, split = "all_materials", 64, 64  # the largest LDS footprint
    gpu, cam = _gpu(hb, name)
    for method in (MIS, NAIVE):
        o = _opts(RAGGED, spp, split, method)
        image = gpu.render(cam, o)[0]
        for kw in MODES:
            got = gpu.render_robust(cam, o, **kw)
            assert got["mean"].tobytes() == image.tobytes()
            assert_robust(got, _expected(name, RAGGED, method, spp, split, **kw), f"S=64 method={method} {kw}")


def test_three_chunks_of_tall_render_tiles_from_pass_five(hb):
    name, spp, split = "overshadowed", 6, 3  # a split that is no power of two
    gpu, cam = _gpu(hb, name)
    o = _opts(RAGGED, spp, split, NAIVE, seed=12, sample_begin=5)
    o.tile_width, o.tile_height = 4, 16  # the work order of the partial buffer follows the render's tiles
    for kw in MODES + (dict(mode=R.GINI, gini_gain=4.0),):
        got = gpu.render_robust(cam, o, **kw)
        assert_robust(got, _expected(name, RAGGED, NAIVE, spp, split, seed=12, sample_begin=5, **kw), f"S=3, tiles 4x16, begin 5 {kw}")
        assert got["mean"].tobytes() == gpu.render(cam, o)[0].tobytes()


def test_two_chunks_are_the_plain_combine_in_every_mode(hb):
    gpu, cam = _gpu(hb, "all_materials")
    o = _opts(RAGGED, 8, 2)
    image = gpu.render(cam, o)[0]
    for kw in (dict(mode=R.TRIM, trim=7), dict(mode=R.MEDIAN), dict(mode=R.GINI, gini_gain=1e6)):
        got = gpu.render_robust(cam, o, **kw)
        finite = got["dropped"] == 0
        assert got["out"][finite].tobytes() == image[finite].tobytes() and not got["trimmed"].any()
        assert_robust(got, _expected("all_materials", RAGGED, MIS, 8, 2, **kw), f"S=2 {kw}")


def test_the_automatic_split_is_reported_and_used(hb):
    name, spp = "spheres500", 32
    gpu, cam = _gpu(hb, name)
    o = _opts(RAGGED, spp, 0)
    got = gpu.render_robust(cam, o, mode="median")
    split = gpu.last_launch_info()["sample_split"]
    auto = gpu.auto_sample_split(o)
    while spp % auto:
        auto //= 2
    print(f"automatic split of {spp} passes at {RAGGED}: {split}")
    assert split == auto and 2 <= split <= 64
    assert_robust(got, _expected(name, RAGGED, MIS, spp, split, mode=R.MEDIAN), f"automatic split {split}")
    o.sample_split = split
    assert got["mean"].tobytes() == gpu.render(cam, o)[0].tobytes()


# ---- rt_robust_combine on synthetic planes ----
def _sums(split, w, h, seed=0, lo=0.0, hi=4.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (split, h, w, 3)).astype(F32)


def _combine_device(hb, gpu, sums, n, albedo=None, off=1, channels=PLANES, stream=0, **kw):
    import torch
    split, h, w = sums.shape[:3]
    run = DeviceRobust(torch, w, h, off=off)
    d_sums = torch.from_numpy(np.ascontiguousarray(sums)).to("cuda:0")
    d_alb = torch.from_numpy(np.ascontiguousarray(albedo)).to("cuda:0") if albedo is not None else None
    torch.cuda.synchronize()
    gpu.robust_combine_device(d_sums.data_ptr(), split, n, w, h, run.ptrs(channels), d_albedo=d_alb.data_ptr() if d_alb is not None else None,
                              stream=stream, **kw)
    torch.cuda.synchronize()
    return run.read_all(channels)


def _check_combine(hb, gpu, sums, n, what, albedo=None, **kw):
    ref = R.robust(sums, n, albedo, **kw)
    assert_robust(_combine_device(hb, gpu, sums, n, albedo, **kw), ref, f"{what} device {kw}")
    assert_robust(gpu.robust_combine(sums, n, albedo=albedo, **kw), ref, f"{what} host {kw}")
    return ref


def test_combine_hand_cases(hb):
    gpu, _ = _gpu(hb, "emit_scene")
    grey = lambda values: np.repeat(np.asarray(values, F32)[:, None, None, None], 3, axis=3)  # noqa: E731
    # one outlier among zeros at S = 8 and S = 4; equal chunks; an all-black pixel; -0 below +0: one pixel each, side by side
    eight = np.concatenate([grey([0, 0, 1024.0, 0, 0, 0, 0, 0]), grey([0.5] * 8), grey([0.0] * 8), grey([0.0, -0.0] * 4)], axis=2)
    for kw in MODES + (dict(mode=R.GINI, gini_gain=0.5), dict(mode=R.GINI, gini_gain=100.0), dict(mode=R.TRIM, trim=0)):
        ref = _check_combine(hb, gpu, eight, 1, "S=8 hand cases", **kw)
        if kw == dict(mode=R.GINI):
            assert ref["trimmed"][0].tolist() == [2, 0, 0, 0] and ref["gini"][0, 2] == 0.0
    four = np.concatenate([grey([0, 7.0, 0, 0]), grey([3.0, 1.0, 2.0, 1.0])], axis=2)
    for kw in MODES:
        ref = _check_combine(hb, gpu, four, 5, "S=4 hand cases", **kw)
    assert ref["trimmed"][0].tolist() == [0, 0]
    # S = 3 under MEDIAN is the middle chunk's sum / n
    three = _sums(3, 5, 4, seed=1)
    ref = _check_combine(hb, gpu, three, 4, "S=3", mode=R.MEDIAN)
    middle = np.argsort(R.luminances(three, 4), axis=0, kind="stable")[1]
    assert ref["out"].tobytes() == (np.take_along_axis(three, middle[None, ..., None], axis=0)[0] / F32(4)).tobytes()


def test_combine_negative_luminances_and_an_albedo(hb):
    gpu, _ = _gpu(hb, "emit_scene")
    sums = _sums(8, 7, 5, seed=2, lo=-3.0, hi=3.0)
    albedo = np.random.default_rng(3).uniform(0.0, 1.0, (5, 7, 3)).astype(F32)
    albedo[1, 1] = 0.0  # floored to 1e-3
    for kw in MODES:
        ref = _check_combine(hb, gpu, sums, 3, "negative luminances", **kw)
        assert (R.luminances(sums, 3) < 0).any() and (ref["G"] < 0).any()
        _check_combine(hb, gpu, sums, 3, "negative luminances, albedo", albedo=albedo, **kw)


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_poisoned_pixel_leaves_its_neighbours_alone(hb, poison):
    gpu, _ = _gpu(hb, "emit_scene")
    sums = _sums(8, 9, 6, seed=4)
    clean = R.robust(sums, 2)
    bad = sums.copy()
    bad[5, 2, 3, 1] = poison      # one chunk of pixel (2, 3)
    bad[:, 4, 8, 0] = poison      # every chunk of pixel (4, 8)
    bad[0:7, 0, 0, 2] = poison    # all but one chunk of pixel (0, 0)
    for kw in MODES:
        ref = _check_combine(hb, gpu, bad, 2, f"poison {poison}", **kw)
        assert (ref["dropped"][2, 3], ref["dropped"][4, 8], ref["dropped"][0, 0]) == (1, 8, 7) and ref["dropped"].sum() == 16
        assert np.isfinite(ref["out"][2, 3]).all() and np.isfinite(ref["out"][0, 0]).all() and not np.isfinite(ref["out"][4, 8]).all()
        assert ref["out"][0, 0].tobytes() == (bad[7, 0, 0] / F32(2)).tobytes() and ref["trimmed"][4, 8] == 0
    untouched = np.ones((6, 9), bool)
    untouched[2, 3] = untouched[4, 8] = untouched[0, 0] = False
    got = gpu.robust_combine(bad, 2)
    for k in PLANES:
        assert got[k][untouched].tobytes() == clean[k][untouched].tobytes(), k


@pytest.mark.parametrize("w,h,split", [(1, 1, 2), (1, 1, 64), (70, 3, 5), (40000, 1, 3)])
def test_combine_frame_shapes(hb, w, h, split):
    """one pixel; 70 x 3, neither side a multiple of anything; a strip of several hundred workgroups"""
    gpu, _ = _gpu(hb, "emit_scene")
    sums = _sums(split, w, h, seed=5)
    sums[split - 1, h - 1, w - 1] *= F32(1e4)  # a firefly in the very last pixel
    for kw in (dict(mode=R.MEDIAN), dict(mode=R.GINI)):
        _check_combine(hb, gpu, sums, 7, f"{w}x{h} S={split}", **kw)
    only_out = _combine_device(hb, gpu, sums, 7, channels=("out",), mode=R.MEDIAN)
    assert_robust(only_out, R.robust(sums, 7, mode=R.MEDIAN), "out alone", ("out",))


def test_raising_the_top_chunk_leaves_the_output_bit_identical(hb):
    gpu, _ = _gpu(hb, "emit_scene")
    sums = _sums(8, 6, 5, seed=6)
    top = np.argmax(R.robust(sums, 2, mode=R.MEDIAN)["ranks"], axis=0)
    idx = np.indices(top.shape)
    raised = sums.copy()
    raised[top, idx[0], idx[1]] = sums[top, idx[0], idx[1]] * F32(1e30)
    for kw in (dict(mode="trim", trim=1), dict(mode="median")):
        a, b = gpu.robust_combine(sums, 2, **kw), gpu.robust_combine(raised, 2, **kw)
        assert a["out"].tobytes() == b["out"].tobytes() and a["mean"].tobytes() != b["mean"].tobytes()


# ---- the pipeline ----
def test_denoised_robust_is_the_aovs_the_robust_frame_and_the_filter(hb):
    import torch
    name, spp, split = "all_materials", 16, 8
    gpu, cam = _gpu(hb, name)
    w, h = WHOLE
    o = _opts(WHOLE, spp, split)
    clean, robust, rays = gpu.render_denoised_robust(cam, o, mode="median")
    assert rays == gpu.render(cam, o)[1] and gpu.last_launch_info()["sample_split"] == split
    aov = gpu.render_aov(cam, o, channels=("albedo", "normal", "depth"))
    one = gpu.render_robust(cam, o, albedo=aov["albedo"], channels=(), mode="median")
    assert robust.tobytes() == one["out"].tobytes()
    assert_same_bits(robust, _expected(name, WHOLE, MIS, spp, split, aov["albedo"], mode=R.MEDIAN)["out"], "robust", nan_equal=True)
    dopts = hb.denoise_opts(w, h)
    planes = {"color": robust, "albedo": aov["albedo"], "normal": aov["normal"], "depth": aov["depth"]}
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in planes.items()}
    ws = torch.zeros(hb.denoise_workspace_bytes(dopts), dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.denoise_device({k: t.data_ptr() for k, t in d.items()}, ws.data_ptr(), d_out.data_ptr(), dopts)
    torch.cuda.synchronize()
    assert clean.tobytes() == d_out.cpu().numpy().tobytes() and clean.tobytes() != robust.tobytes()
    only_clean = gpu.render_denoised_robust(cam, o, mode="median")[0]
    assert only_clean.tobytes() == clean.tobytes()


def test_a_captured_second_call_replays_the_eager_bytes(hb):
    """the first call grows the scene's scratch (no `mean` is given, so the render goes there); the second is captured and
    replayed twice"""
    import torch
    name, spp, split = "all_materials", 8, 4
    gpu, cam = _gpu(hb, name)
    w, h = RAGGED
    o = _opts(RAGGED, spp, split)
    dev = torch.device("cuda", 0)
    channels = ("out", "gini", "trimmed", "dropped")
    eager = DeviceRobust(torch, w, h)
    torch.cuda.synchronize()
    gpu.render_robust_device(cam, o, eager.ptrs(channels), d_rays_ptr=eager.rays.data_ptr(), mode="median")
    torch.cuda.synchronize()
    ref = eager.read_all(channels)
    assert eager.untouched("mean")
    assert_robust(ref, _expected(name, RAGGED, MIS, spp, split, mode=R.MEDIAN), "eager", channels)
    run = DeviceRobust(torch, w, h)
    g = capture(torch, lambda stream: gpu.render_robust_device(cam, o, run.ptrs(channels), d_rays_ptr=run.rays.data_ptr(), stream=stream,
                                                                mode="median"))
    assert all(run.untouched(k) for k in run.buf)  # capture ran nothing
    for replay in range(2):
        run.rays.zero_()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        assert_robust(run.read_all(channels), ref, f"replay {replay}", channels)
        assert int(run.rays.item()) == int(eager.rays.item())
    # rt_robust_combine_device keeps no state: captured as the first call of its kind on a scene of its own
    fresh, _ = _gpu(hb, name)
    sums = _sums(4, w, h, seed=7)
    d_sums = torch.from_numpy(sums).to("cuda:0")
    comb = DeviceRobust(torch, w, h)
    g = capture(torch, lambda stream: fresh.robust_combine_device(d_sums.data_ptr(), 4, 2, w, h, comb.ptrs(), stream=stream, mode="median"))
    assert all(comb.untouched(k) for k in comb.buf)
    g.replay()
    torch.cuda.synchronize(dev)
    assert_robust(comb.read_all(), R.robust(sums, 2, mode=R.MEDIAN), "captured combine")


def test_a_following_render_returns_the_same_bytes(hb):
    gpu, cam = _gpu(hb, "overshadowed")
    opts = abi.default_render_opts(96, 54, 8, method=MIS, seed=2)
    img_a, rays_a = gpu.render(cam, opts)
    info_a = gpu.last_launch_info()
    o = _opts((96, 54), 8, 4, seed=2)
    gpu.render_robust(cam, o)
    info_robust = gpu.last_launch_info()
    gpu.render(cam, o)
    assert gpu.last_launch_info() == info_robust  # describes the render launch of the robust call
    gpu.robust_combine(_sums(4, 96, 54), 2)
    assert gpu.last_launch_info() == info_robust  # the combine alone launches no render
    gpu.render_denoised_robust(cam, o)
    img_b, rays_b = gpu.render(cam, opts)
    assert np.array_equal(img_a, img_b) and rays_a == rays_b and gpu.last_launch_info() == info_a


def test_a_multi_device_head_is_refused(hb):
    sc, cam_params, _, _ = _built("all_materials")
    multi = hb.HipScene(sc, devices=[0, 0])
    cam = hb.camera_new(**cam_params)
    o = _opts(RAGGED, 8, 4)
    for call in (lambda: multi.render_robust(cam, o), lambda: multi.render_denoised_robust(cam, o)):
        with pytest.raises(hb.RtHipError) as e:
            call()
        assert e.value.code == abi.RT_ERR_UNSUPPORTED
    # the caller's own chunk sums are no render: the head combines them on its first device
    sums = _sums(4, *RAGGED, seed=8)
    assert_robust(multi.robust_combine(sums, 2), R.robust(sums, 2), "combine on a multi-device head")
