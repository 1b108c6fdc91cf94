"""The noise estimates on the GPU against the numpy checker (tests/noise_checker.py): rt_render_noise[_device], rt_noise_tiles[_device],
rt_render_converged and rt_render_denoised_split.  Every comparison is bit for bit (NaN == NaN).  The passes of a scene come from
the CPU oracle once per (scene, frame, method, window) and are shared."""
import functools

import numpy as np
import pytest

import aov_checker as K
import noise_checker as N
import scenes
from gpu_support import GuardedBuffers, assert_same_bits, capture, ssml_scene

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
SEED = 3
WHOLE, RAGGED = (24, 20), (13, 11)  # whole and half tiles; ragged on both axes
MIS, NAIVE = abi.RT_METHOD_MIS, abi.RT_METHOD_NAIVE


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


def _expected(name, size, method, spp, split, albedo=None, seed=SEED, sample_begin=0, **nopts):
    mean, lbar, var = N.estimate(N.chunk_sums(_passes(name, size, method, seed, sample_begin, spp), split), spp, albedo)
    err, summary = N.tiles(lbar, var, **nopts)
    return {"mean": mean, "lum_mean": lbar, "variance": var, "tile_error": err, "summary": summary}


def _gpu(hb, name):
    sc, cam_params, _, _ = _built(name)
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


def assert_summary(got, ref, what):
    assert_same_bits(np.asarray([got["max_tile_error"]], F32), np.asarray([ref["max_tile_error"]], F32), f"{what} max_tile_error", nan_equal=True)
    assert (got["tiles_above"], got["n_tiles"]) == (ref["tiles_above"], ref["n_tiles"]), (what, got, ref)


def assert_estimate(got, ref, what, channels=("mean", "variance", "lum_mean", "tile_error")):
    for name in channels:
        assert_same_bits(got[name], ref[name], f"{what} {name}", nan_equal=True)
    assert_summary(got["summary"], ref["summary"], what)


class DeviceNoise(GuardedBuffers):
    """the five outputs in device memory, each with guard values before and after, and the ray counter"""

    def __init__(self, torch, w, h):
        ty, tx = (h + 7) // 8, (w + 7) // 8
        super().__init__(torch, {"mean": ((h, w, 3), F32), "variance": ((h, w), F32), "lum_mean": ((h, w), F32),
                                 "tile_error": ((ty, tx), F32), "summary": ((4,), np.uint32)})
        self.rays = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def read_estimate(self):
        res = self.read_all()
        s = res["summary"]
        assert s[3] == 0, "the reserved word of the summary"
        res["summary"] = {"max_tile_error": s[:1].view(np.float32)[0], "tiles_above": int(s[1]), "n_tiles": int(s[2])}
        return res


# ---- one render: every scene, both methods ----
@pytest.mark.parametrize("method", [MIS, NAIVE])
@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_match_the_checker(hb, name, method):
    gpu, cam = _gpu(hb, name)
    spp = 8
    albedo = gpu.render_aov(cam, _opts(WHOLE, spp, 1, method), channels=("albedo",))["albedo"]
    noisy = 0
    for split in (2, 4, 8):
        o = _opts(WHOLE, spp, split, method)
        got = gpu.render_noise(cam, o)
        image, rays = gpu.render(cam, o)
        assert got["mean"].tobytes() == image.tobytes() and got["rays_shot"] == rays, f"{name} S={split}: not the bytes of rt_render"
        assert gpu.last_launch_info()["sample_split"] == split
        ref = _expected(name, WHOLE, method, spp, split)
        assert_estimate(got, ref, f"{name} method={method} S={split}")
        noisy += int((ref["variance"] > 0).sum())
        with_albedo = gpu.render_noise(cam, o, albedo=albedo)
        assert_estimate(with_albedo, _expected(name, WHOLE, method, spp, split, albedo), f"{name} method={method} S={split} albedo")
        assert with_albedo["mean"].tobytes() == image.tobytes()
    assert noisy > 50, "a frame without noise would test nothing"


@pytest.mark.parametrize("split", [2, 4, 8])
def test_a_ragged_frame_through_the_host_and_the_device_entry(hb, split):
    import torch
    name, spp = "all_materials", 8
    gpu, cam = _gpu(hb, name)
    w, h = RAGGED
    o = _opts(RAGGED, spp, split)
    albedo = gpu.render_aov(cam, o, channels=("albedo",))["albedo"]
    d_albedo = torch.from_numpy(albedo).to("cuda:0")
    d_frame = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda:0")
    gpu.render_device(cam, o, d_frame.data_ptr())
    torch.cuda.synchronize()
    frame = d_frame.cpu().numpy().reshape(h, w, 3)
    for alb, d_alb in ((None, None), (albedo, d_albedo.data_ptr())):
        ref = _expected(name, RAGGED, MIS, spp, split, alb)
        assert ref["mean"].tobytes() == frame.tobytes()  # the checker's combine is rt_render_device's
        assert_estimate(gpu.render_noise(cam, o, albedo=alb), ref, f"host S={split} albedo={alb is not None}")
        run = DeviceNoise(torch, w, h)
        torch.cuda.synchronize()
        gpu.render_noise_device(cam, o, run.ptrs(), d_albedo=d_alb, d_rays_ptr=run.rays.data_ptr())
        torch.cuda.synchronize()
        got = run.read_estimate()
        assert_estimate(got, ref, f"device S={split} albedo={alb is not None}")
        assert got["mean"].tobytes() == frame.tobytes() and int(run.rays.item()) == gpu.render(cam, o)[1]
        # the tile outputs without the planes they are made from, and the mean alone
        for channels in (("mean", "tile_error", "summary"), ("mean", "summary"), ("mean",), ("mean", "variance")):
            part = DeviceNoise(torch, w, h)
            torch.cuda.synchronize()
            gpu.render_noise_device(cam, o, part.ptrs(channels), d_albedo=d_alb)
            torch.cuda.synchronize()
            for k in abi.NOISE_CHANNELS:
                if k in channels:
                    assert part.read(k).tobytes() == run.read(k).tobytes(), (channels, k)
                else:
                    assert part.untouched(k), f"{k} was written though not asked for"
    host_only_mean = gpu.render_noise(cam, o, channels=())
    assert set(host_only_mean) == {"mean", "rays_shot"} and host_only_mean["mean"].tobytes() == frame.tobytes()


def test_sixty_four_chunks_of_one_pass(hb):
    name, spp, split = "all_materials", 64, 64
    gpu, cam = _gpu(hb, name)
    for method in (MIS, NAIVE):
        o = _opts(RAGGED, spp, split, method)
        got = gpu.render_noise(cam, o)
        assert got["mean"].tobytes() == gpu.render(cam, o)[0].tobytes()
        assert_estimate(got, _expected(name, RAGGED, method, spp, split), f"S=64 method={method}")


def test_the_automatic_split_is_reported_and_used(hb):
    name, spp = "spheres500", 32
    gpu, cam = _gpu(hb, name)
    o = _opts(RAGGED, spp, 0)
    got = gpu.render_noise(cam, o)
    split = gpu.last_launch_info()["sample_split"]
    auto = gpu.auto_sample_split(o)
    while spp % auto:
        auto //= 2
    print(f"automatic split of {spp} passes at {RAGGED}: {split}")
    assert split == auto and 2 <= split <= 64
    assert_estimate(got, _expected(name, RAGGED, MIS, spp, split), f"automatic split {split}")
    o.sample_split = split
    assert got["mean"].tobytes() == gpu.render(cam, o)[0].tobytes()


def test_non_default_options_and_a_window_that_starts_at_pass_five(hb):
    name, spp, split = "overshadowed", 6, 3  # a split that is no power of two
    gpu, cam = _gpu(hb, name)
    o = _opts(RAGGED, spp, split, NAIVE, seed=12, sample_begin=5)
    o.tile_width, o.tile_height = 4, 16  # the render's own tiles are not the error map's
    got = gpu.render_noise(cam, o, luminance_floor=0.5, threshold=0.125)
    ref = _expected(name, RAGGED, NAIVE, spp, split, seed=12, sample_begin=5, luminance_floor=0.5, threshold=0.125)
    assert_estimate(got, ref, "S=3, tiles 4x16, begin 5")
    assert got["mean"].tobytes() == gpu.render(cam, o)[0].tobytes()


# ---- the tile stage on synthetic planes ----
def _planes(w, h, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 2.0, (h, w)).astype(F32), (rng.uniform(0.0, 0.2, (h, w)) ** 2).astype(F32)


def _tiles_device(hb, gpu, lum, var, **nopts):
    import torch
    h, w = lum.shape
    run = DeviceNoise(torch, w, h)
    d_lum, d_var = torch.from_numpy(lum).to("cuda:0"), torch.from_numpy(var).to("cuda:0")
    torch.cuda.synchronize()
    gpu.noise_tiles_device(d_lum.data_ptr(), d_var.data_ptr(), w, h, run.ptrs()["tile_error"], run.ptrs()["summary"], **nopts)
    torch.cuda.synchronize()
    got = run.read_estimate()
    return got["tile_error"], got["summary"]


def test_tiles_that_hold_a_non_finite_pixel_report_infinity(hb):
    """a NaN variance, an infinite variance, a negative variance and a NaN lum_mean, each in a tile of its own, make that tile
    +inf; a NEGATIVE lum_mean, in a fifth tile, enters by its absolute value as the definition says (r = sqrtf(variance) /
    (fabsf(lum_mean) + luminance_floor)): that tile is finite and equals the tile with the sign removed"""
    gpu, _ = _gpu(hb, "emit_scene")
    w, h = 45, 27  # 6 x 4 tiles, ragged on both axes
    lum, var = _planes(w, h)
    clean, clean_summary = N.tiles(lum, var)
    var[3, 4] = np.nan       # tile (0, 0)
    var[9, 20] = np.inf      # tile (2, 1)
    var[26, 44] = -1.0       # tile (5, 3), the ragged corner
    lum[17, 30] = np.nan     # tile (3, 2)
    lum[12, 2] = -lum[12, 2]  # tile (0, 1)
    bad = [(0, 0), (1, 2), (3, 5), (2, 3)]
    ref, ref_summary = N.tiles(lum, var)
    assert all(ref[t] == np.inf for t in bad) and ref_summary["max_tile_error"] == np.inf and np.isfinite(ref).sum() == 24 - 4
    assert ref[1, 0] == clean[1, 0] and np.isfinite(ref[1, 0])
    untouched = np.ones((4, 6), bool)
    for t in bad:
        untouched[t] = False
    assert ref[untouched].tobytes() == clean[untouched].tobytes()
    assert ref_summary["tiles_above"] == int((clean[untouched] > F32(0.05)).sum()) + 4
    for entry in ("device", "host"):
        err, summary = _tiles_device(hb, gpu, lum, var) if entry == "device" else gpu.noise_tiles(lum, var)
        assert_same_bits(err, ref, f"{entry} tile_error", nan_equal=True)
        assert_summary(summary, ref_summary, entry)
        assert summary["max_tile_error"] == np.inf
    err, summary = gpu.noise_tiles(np.abs(np.nan_to_num(lum, nan=1.0)), np.abs(np.nan_to_num(var, nan=0.0, posinf=1.0)))
    assert np.isfinite(err).all() and np.isfinite(summary["max_tile_error"])


def test_a_threshold_equal_to_a_tiles_error_does_not_count_it(hb):
    gpu, _ = _gpu(hb, "emit_scene")
    lum, var = _planes(*RAGGED, seed=1)
    ref, _ = N.tiles(lum, var)
    ranked = np.sort(ref.reshape(-1))
    assert len(np.unique(ranked)) == 4
    pin = float(ranked[1])
    for threshold, above in ((pin, 2), (float(np.nextafter(F32(pin), F32(0))), 3), (0.0, 4), (float(ranked[3]), 0)):
        _, ref_summary = N.tiles(lum, var, threshold=threshold)
        assert ref_summary["tiles_above"] == above
        err, summary = _tiles_device(hb, gpu, lum, var, threshold=threshold)
        assert_same_bits(err, ref, f"threshold {threshold}", nan_equal=True)
        assert_summary(summary, ref_summary, f"threshold {threshold}")
        assert_summary(gpu.noise_tiles(lum, var, threshold=threshold)[1], ref_summary, f"host, threshold {threshold}")


def test_a_strip_with_more_tiles_than_one_pass_of_the_grid(hb):
    """the tile kernel's grid covers abi.NOISE_TILES_PER_GRID_PASS tiles, then it strides: two rows of tiles, 2.0 grid passes and
    a few tiles, the last column and the last row ragged"""
    gpu, _ = _gpu(hb, "emit_scene")
    w, h = 8 * (abi.NOISE_TILES_PER_GRID_PASS + 3) + 5, 11
    lum, var = _planes(w, h, seed=2)
    var[10, w - 1] = np.inf  # the very last tile
    ref, ref_summary = N.tiles(lum, var, luminance_floor=0.02, threshold=0.1)
    assert ref.size == 2 * (abi.NOISE_TILES_PER_GRID_PASS + 4) and 0 < ref_summary["tiles_above"] < ref.size
    err, summary = _tiles_device(hb, gpu, lum, var, luminance_floor=0.02, threshold=0.1)
    assert_same_bits(err, ref, "strip tile_error", nan_equal=True)
    assert_summary(summary, ref_summary, "strip")
    # the summary alone, and a one-pixel frame
    import torch
    d_lum, d_var = torch.from_numpy(lum).to("cuda:0"), torch.from_numpy(var).to("cuda:0")
    d_sum = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    gpu.noise_tiles_device(d_lum.data_ptr(), d_var.data_ptr(), w, h, None, d_sum.data_ptr(), luminance_floor=0.02, threshold=0.1)
    torch.cuda.synchronize()
    s = d_sum.cpu().numpy().view(np.uint32)
    assert (int(s[1]), int(s[2]), int(s[3])) == (ref_summary["tiles_above"], ref.size, 0) and s[:1].view(F32)[0] == np.inf
    one, one_summary = gpu.noise_tiles(np.full((1, 1), 0.99, F32), np.full((1, 1), 4.0, F32))
    assert one.tolist() == [[2.0]] and one_summary == {"max_tile_error": F32(2.0), "tiles_above": 1, "n_tiles": 1}


# ---- render until converged ----
CONV = dict(name="all_materials", size=WHOLE, method=MIS, batch=8, split=2, n=4)


@functools.lru_cache(maxsize=None)
def _converged_reference():
    """the checker's accumulation after 1 .. 4 batches: (mean, lum_mean, variance, tile_error, max_tile_error) each"""
    c = CONV
    batches, out = [], []
    for b in range(c["n"]):
        sums = N.chunk_sums(_passes(c["name"], c["size"], c["method"], SEED, b * c["batch"], c["batch"]), c["split"])
        batches.append(N.estimate(sums, c["batch"]))
        mean, lum, var = N.accumulate(batches)
        out.append((mean, lum, var) + N.tiles(lum, var, threshold=0.0))
    return out


def _converge(gpu, cam, **kw):
    c = CONV
    return gpu.render_converged(cam, _opts(c["size"], 999, c["split"], c["method"]), c["batch"], **kw)


def _assert_converged(got, ref, n_batches, what):
    mean, _, var, err, _ = ref[n_batches - 1]
    assert (got["batches"], got["passes"]) == (n_batches, n_batches * CONV["batch"]), (what, got["batches"], got["passes"])
    assert_same_bits(got["mean"], mean, f"{what} mean", nan_equal=True)
    assert_same_bits(got["variance"], var, f"{what} variance", nan_equal=True)
    assert_same_bits(got["tile_error"], err, f"{what} tile_error", nan_equal=True)


def test_converged_stops_at_the_batch_the_checker_predicts(hb):
    c = CONV
    ref = _converged_reference()
    worst = [float(r[4]["max_tile_error"]) for r in ref]
    print("max_tile_error after 1..4 batches:", worst)
    assert all(np.isfinite(worst)) and max(worst) > min(worst)
    threshold = float(F32(0.5 * (max(worst) + min(worst))))
    stop = next(i for i, e in enumerate(worst) if F32(e) <= F32(threshold)) + 1
    gpu, cam = _gpu(hb, c["name"])
    got = _converge(gpu, cam, max_passes=c["n"] * c["batch"], threshold=threshold)
    _assert_converged(got, ref, stop, f"threshold {threshold}")
    assert got["converged"] == (worst[stop - 1] <= threshold)
    _, ref_summary = N.tiles(ref[stop - 1][1], ref[stop - 1][2], threshold=threshold)
    assert_summary(got["summary"], ref_summary, "the summary of the last batch")
    rays = 0
    for b in range(stop):
        rays += gpu.render(cam, _opts(c["size"], c["batch"], c["split"], c["method"], sample_begin=b * c["batch"]))[1]
    assert got["rays_shot"] == rays
    # min_batches holds it past the batch that was good enough
    if stop < c["n"]:
        held = _converge(gpu, cam, min_batches=stop + 1, max_passes=c["n"] * c["batch"], threshold=max(worst))
        _assert_converged(held, ref, stop + 1, f"min_batches {stop + 1}")
        assert held["converged"]
    loose = _converge(gpu, cam, max_passes=c["n"] * c["batch"], threshold=max(worst))
    _assert_converged(loose, ref, 1, "a threshold every batch meets")
    held = _converge(gpu, cam, min_batches=3, max_passes=c["n"] * c["batch"], threshold=max(worst))
    _assert_converged(held, ref, 3, "min_batches 3")
    assert held["converged"]


def test_threshold_zero_runs_to_max_passes(hb):
    c = CONV
    ref = _converged_reference()
    gpu, cam = _gpu(hb, c["name"])
    got = _converge(gpu, cam, max_passes=c["n"] * c["batch"] + c["batch"] - 1, threshold=0.0)  # a fifth window would exceed it
    _assert_converged(got, ref, c["n"], "threshold 0")
    assert not got["converged"]
    assert_summary(got["summary"], ref[c["n"] - 1][4], "threshold 0")
    # the render's state is as it was found: the next render is what it would have been
    o = _opts(c["size"], 8, 1, c["method"])
    fresh_gpu, _ = _gpu(hb, c["name"])
    assert gpu.render(cam, o)[0].tobytes() == fresh_gpu.render(cam, o)[0].tobytes()


def test_one_batch_is_the_one_shot_call(hb):
    c = CONV
    gpu, cam = _gpu(hb, c["name"])
    got = _converge(gpu, cam, max_passes=c["batch"], threshold=0.0)
    one = gpu.render_noise(cam, _opts(c["size"], c["batch"], c["split"], c["method"]), threshold=0.0)
    assert got["batches"] == 1 and not got["converged"] and got["rays_shot"] == one["rays_shot"]
    for k in ("mean", "variance", "tile_error"):
        assert got[k].tobytes() == one[k].tobytes(), k
    assert_summary(got["summary"], one["summary"], "one batch")
    _assert_converged(got, _converged_reference(), 1, "one batch")


# ---- render + denoise from one render ----
def test_denoised_split_is_one_render_its_variance_and_the_filter(hb):
    import torch
    name, spp, split = "all_materials", 8, 4
    gpu, cam = _gpu(hb, name)
    w, h = WHOLE
    o = _opts(WHOLE, spp, split)
    clean, noisy, variance, rays = gpu.render_denoised_split(cam, o)
    image, image_rays = gpu.render(cam, o)
    assert noisy.tobytes() == image.tobytes() and rays == image_rays
    aov = gpu.render_aov(cam, o, channels=("albedo", "normal", "depth"))
    one = gpu.render_noise(cam, o, albedo=aov["albedo"], channels=("variance",))
    assert variance.tobytes() == one["variance"].tobytes()
    assert_same_bits(variance, _expected(name, WHOLE, MIS, spp, split, aov["albedo"])["variance"], "variance", nan_equal=True)
    dopts = hb.denoise_opts(w, h)
    planes = {"color": noisy, "albedo": aov["albedo"], "normal": aov["normal"], "depth": aov["depth"], "variance": variance}
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in planes.items()}
    ws = torch.zeros(hb.denoise_workspace_bytes(dopts), dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.denoise_device({k: t.data_ptr() for k, t in d.items()}, ws.data_ptr(), d_out.data_ptr(), dopts)
    torch.cuda.synchronize()
    assert clean.tobytes() == d_out.cpu().numpy().tobytes()
    assert clean.tobytes() != noisy.tobytes()
    assert gpu.last_launch_info()["sample_split"] == split


# ---- graph capture, side effects ----
def test_a_captured_second_call_replays_the_eager_bytes(hb):
    """the first call grows the scene's scratch; the second is captured and replayed twice WITHOUT clearing the summary in
    between: a summary that is not reset by the graph would count its tiles twice"""
    import torch
    name, spp, split = "all_materials", 8, 4
    gpu, cam = _gpu(hb, name)
    w, h = RAGGED
    o = _opts(RAGGED, spp, split)
    dev = torch.device("cuda", 0)
    eager = DeviceNoise(torch, w, h)
    torch.cuda.synchronize()
    gpu.render_noise_device(cam, o, eager.ptrs(), d_rays_ptr=eager.rays.data_ptr(), threshold=0.01)
    torch.cuda.synchronize()
    ref = eager.read_estimate()
    assert ref["summary"]["tiles_above"] > 0
    assert_estimate(ref, _expected(name, RAGGED, MIS, spp, split, threshold=0.01), "eager")
    run = DeviceNoise(torch, w, h)
    g = capture(torch, lambda stream: gpu.render_noise_device(cam, o, run.ptrs(), d_rays_ptr=run.rays.data_ptr(), stream=stream,
                                                               threshold=0.01))
    assert all(run.untouched(k) for k in run.buf)  # capture ran nothing
    for replay in range(2):
        run.rays.zero_()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        got = run.read_estimate()
        assert_estimate(got, ref, f"replay {replay}")
        assert int(run.rays.item()) == int(eager.rays.item())


def test_a_following_render_returns_the_same_bytes(hb):
    gpu, cam = _gpu(hb, "overshadowed")
    opts = abi.default_render_opts(96, 54, 8, method=MIS, seed=2)
    img_a, rays_a = gpu.render(cam, opts)
    info_a = gpu.last_launch_info()
    o = _opts((96, 54), 8, 4, seed=2)
    gpu.render_noise(cam, o)
    info_noise = gpu.last_launch_info()
    gpu.render(cam, o)
    assert gpu.last_launch_info() == info_noise  # describes the render launch of the noise call
    gpu.render_converged(cam, o, 8, max_passes=16, threshold=0.0)
    gpu.render_denoised_split(cam, o)
    gpu.noise_tiles(np.ones((54, 96), F32), np.ones((54, 96), F32))
    img_b, rays_b = gpu.render(cam, opts)
    assert np.array_equal(img_a, img_b) and rays_a == rays_b and gpu.last_launch_info() == info_a
