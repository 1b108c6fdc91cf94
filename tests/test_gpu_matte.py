"""Anti-aliased ID mattes (rt_render_matte, rt_matte_extract) on the GPU.  Everything is counting, so every comparison is bit for
bit: the layers against tests/matte_checker.py fed with the library's own per-pass IDs (16 single-pass rt_render_aov calls) and
with the oracle's, the mattes against the checker's extraction."""
import functools

import numpy as np
import pytest

import aov_checker as K
import matte_checker as M
import scenes
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture, ssml_scene

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
W, H, SPP = 64, 36, 16
SKY = abi.AOV_NO_ID
KINDS = ("primitive", "material")
OUTPUTS = ("ids", "coverage", "residual")  # of rt_render_matte_device


SCENES = {
    "emit_scene": lambda: (K.emit_scene(), K.EMIT_CAMERA),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "spheres500": lambda: (scenes.random_spheres(500), scenes.MESH_CAMERA),
    "mesh2000": lambda: (scenes.random_triangle_mesh(2000), scenes.MESH_CAMERA),
    "pyramid": lambda: ssml_scene("pyramid"),
    # triangles two units wide: a pixel of a 16 x 9 frame sees more than eight of them (the overflow case; chosen with the oracle)
    "mesh2000_wide": lambda: (scenes.random_triangle_mesh(2000, edge=2.0), scenes.MESH_CAMERA),
}


@functools.lru_cache(maxsize=None)
def _scene(hb, name):
    sc, cam_params = SCENES[name]()
    return sc, cam_params, hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


def _opts(w, h, spp, seed, sample_begin=0):
    o = abi.default_render_opts(w, h, spp, seed=seed)
    o.sample_begin = sample_begin
    return o


@functools.lru_cache(maxsize=None)
def _own_pass_ids(hb, name, kind, w, h, spp, seed, sample_begin):
    """[spp, w*h] u32: the `kind` channel of rt_render_aov for each single pass of the window (computed once, never written to)"""
    _, _, gpu, cam = _scene(hb, name)
    out = np.stack([gpu.render_aov(cam, _opts(w, h, 1, seed, sample_begin + p), channels=(kind,))[kind].reshape(-1) for p in range(spp)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(hb, name, kind, w, h, spp, seed, sample_begin, layers=8):
    ref = M.layers_from_pass_ids(_own_pass_ids(hb, name, kind, w, h, spp, seed, sample_begin), layers)
    for a in ref:
        a.setflags(write=False)
    return ref


def assert_layers_equal(got, ref, what):
    """got: the dict of HipScene.render_matte; ref: the checker's flat (ids, coverage, residual)"""
    k, h, w = got["ids"].shape
    assert_same_bits(got["ids"].reshape(k, -1), ref[0], f"{what} ids", nan_equal=False)
    assert_same_bits(got["coverage"].reshape(k, -1), ref[1], f"{what} coverage", nan_equal=False)
    if "residual" in got:
        assert_same_bits(got["residual"].reshape(-1), ref[2], f"{what} residual", nan_equal=False)


# ---- the layers ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["emit_scene", "all_materials", "spheres500", "mesh2000", "pyramid"])
def test_layers_match_the_librarys_own_pass_ids(hb, name, kind):
    _, _, gpu, cam = _scene(hb, name)
    ref = _reference(hb, name, kind, W, H, SPP, 3, 0)
    opts = _opts(W, H, SPP, 3)
    try:
        for mode in (0, 1):  # exhaustive / pruned: the same bytes
            gpu.set_traversal(mode)
            assert_layers_equal(gpu.render_matte(cam, opts, id_kind=kind, layers=8, residual=True), ref, f"{name} {kind} traversal={mode}")
    finally:
        gpu.set_traversal(-1)
    assert_layers_equal(gpu.render_matte(cam, opts, id_kind=kind, layers=8, residual=True), ref, f"{name} {kind} auto traversal")
    assert (ref[1][0] > 0).all() and (ref[1][0] < 1).any()  # every pixel has a first rank, and some pixel shares itself out


@pytest.mark.parametrize("name", ["all_materials", "spheres500"])
def test_layers_match_the_oracle(hb, O, name):
    sc, cam_params, gpu, cam = _scene(hb, name)
    cpu, cam_c = O.Scene(sc), O.camera_new(**cam_params)
    pixels = K.tile_pixels(W, H, [(0, 0), (3, 2), (7, 4)])  # the last one is an edge tile: 36 = 4 * 8 + 4
    for kind in KINDS:
        ref = M.layers_from_pass_ids(M.pass_ids(sc, cpu, cam_c, W, H, SPP, 3, 0, kind, pixels=pixels), 8)
        got = gpu.render_matte(cam, _opts(W, H, SPP, 3), id_kind=kind, layers=8, residual=True)
        assert_same_bits(got["ids"].reshape(8, -1)[:, pixels], ref[0], f"{name} {kind} ids", nan_equal=False)
        assert_same_bits(got["coverage"].reshape(8, -1)[:, pixels], ref[1], f"{name} {kind} coverage", nan_equal=False)
        assert_same_bits(got["residual"].reshape(-1)[pixels], ref[2], f"{name} {kind} residual", nan_equal=False)


def test_overflow_is_exercised(hb):
    """16 x 9 x 64 passes over wide triangles: pixels see more than eight primitives, and IDs that came too late come again"""
    w, h, spp = 16, 9, 64
    passes = _own_pass_ids(hb, "mesh2000_wide", "primitive", w, h, spp, 7, 0)
    crowded = late_again = 0
    for q in range(w * h):
        order = list(dict.fromkeys(passes[:, q].tolist()))  # distinct IDs in order of arrival
        crowded += len(order) > 8
        late_again += any((passes[:, q] == v).sum() > 1 for v in order[8:])
    assert crowded >= 4 and late_again >= 1, (crowded, late_again)
    _, _, gpu, cam = _scene(hb, "mesh2000_wide")
    ref = _reference(hb, "mesh2000_wide", "primitive", w, h, spp, 7, 0)
    got = gpu.render_matte(cam, _opts(w, h, spp, 7), id_kind="primitive", layers=8, residual=True)
    assert_layers_equal(got, ref, "overflow")
    assert (got["residual"] > 0).sum() >= crowded  # with eight layers the residual is exactly the overflow


def test_power_of_two_passes_are_exact(hb):
    _, _, gpu, cam = _scene(hb, "spheres500")
    for kind in KINDS:
        got = gpu.render_matte(cam, _opts(W, H, 16, 3), id_kind=kind, layers=8, residual=True)
        counts = got["coverage"] * F32(16)
        assert (counts == np.round(counts)).all() and (got["coverage"] >= 0).all() and not np.signbit(got["coverage"]).any()
        total = got["residual"].copy()
        for l in range(8):
            total = total + got["coverage"][l]
        assert total.dtype == np.float32 and (total == F32(1.0)).all()
        empty = got["coverage"] == 0
        assert (got["ids"][empty] == SKY).all()  # an empty layer reads (UINT32_MAX, +0)
        assert (np.diff(got["coverage"], axis=0) <= 0).all()  # ranked


@pytest.mark.parametrize("kind", KINDS)
def test_fewer_layers_are_prefixes(hb, kind):
    _, _, gpu, cam = _scene(hb, "mesh2000_wide")
    opts = _opts(32, 18, 16, 11)
    full = gpu.render_matte(cam, opts, id_kind=kind, layers=8, residual=True)
    assert_layers_equal(full, _reference(hb, "mesh2000_wide", kind, 32, 18, 16, 11, 0), f"{kind} K=8")
    previous = full["residual"]
    for k in range(7, 0, -1):
        got = gpu.render_matte(cam, opts, id_kind=kind, layers=k, residual=True)
        assert got["ids"].shape == got["coverage"].shape == (k, 18, 32)
        assert_same_bits(got["ids"], full["ids"][:k], f"{kind} K={k} ids", nan_equal=False)
        assert_same_bits(got["coverage"], full["coverage"][:k], f"{kind} K={k} coverage", nan_equal=False)
        assert_same_bits(got["residual"], (previous + full["coverage"][k]).astype(np.float32), f"{kind} K={k} residual", nan_equal=False)  # sixteenths: exact
        assert (got["residual"] >= previous).all()
        previous = got["residual"]
    if kind == "primitive":
        assert (previous > full["residual"]).any()


def test_a_window_that_does_not_start_at_zero(hb):
    _, _, gpu, cam = _scene(hb, "all_materials")
    for kind in KINDS:
        ref = _reference(hb, "all_materials", kind, W, H, SPP, 9, 5)
        assert_layers_equal(gpu.render_matte(cam, _opts(W, H, SPP, 9, 5), id_kind=kind, layers=8, residual=True), ref, f"sample_begin=5 {kind}")
    # (another window is another jitter: not the bytes of the window that starts at pass 0)
    assert _reference(hb, "all_materials", "primitive", W, H, SPP, 9, 5)[1].tobytes() != _reference(hb, "all_materials", "primitive", W, H, SPP, 9, 0)[1].tobytes()


@pytest.mark.parametrize("w,h", [(37, 21), (2, 2)])
def test_ragged_and_tiny_frames(hb, w, h):
    _, _, gpu, cam = _scene(hb, "spheres500")
    for kind in KINDS:
        ref = _reference(hb, "spheres500", kind, w, h, 8, 4, 0)
        assert_layers_equal(gpu.render_matte(cam, _opts(w, h, 8, 4), id_kind=kind, layers=8, residual=True), ref, f"{w}x{h} {kind}")


def device_matte(torch, w, h, layers=8):
    """the three output buffers on the device between guard words (a NaN pattern: the strict compare tells it from any output), and
    a matte behind them"""
    return GuardedBuffers(torch, {"ids": ((layers, h, w), np.uint32), "coverage": ((layers, h, w), np.float32),
                                  "residual": ((h, w), np.float32), "matte": ((h, w), np.float32)}, guard=0x7FC0BEEF)


def test_without_the_residual_nothing_is_written_to_it(hb):
    import torch
    _, _, gpu, cam = _scene(hb, "all_materials")
    opts = _opts(37, 21, 8, 2)
    ref = gpu.render_matte(cam, opts, layers=3, residual=True)
    run = device_matte(torch, 37, 21)
    torch.cuda.synchronize()
    gpu.render_matte_device(cam, opts, run.ptrs(("ids", "coverage")), layers=3)
    torch.cuda.synchronize()
    assert run.untouched("residual")
    assert_same_bits(run.read("ids", used=3 * 37 * 21), ref["ids"], "ids", nan_equal=False)  # (read() checks that layers 3 .. 7 still hold the guard)
    assert_same_bits(run.read("coverage", used=3 * 37 * 21), ref["coverage"], "coverage", nan_equal=False)
    host = gpu.render_matte(cam, opts, layers=3)
    assert set(host) == {"ids", "coverage"}
    assert_same_bits(host["ids"], ref["ids"], "host call without the residual", nan_equal=False)


def test_host_call_device_call_streams_and_a_multi_device_head_agree(hb):
    import torch
    sc, _, gpu, cam = _scene(hb, "spheres500")
    opts = _opts(W, H, SPP, 3)
    ref = _reference(hb, "spheres500", "primitive", W, H, SPP, 3, 0)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    for stream in (0, side.cuda_stream):
        run = device_matte(torch, W, H)
        torch.cuda.synchronize()
        gpu.render_matte_device(cam, opts, run.ptrs(OUTPUTS), id_kind="primitive", layers=8, stream=stream)
        torch.cuda.synchronize()
        got = run.read_all(OUTPUTS)
        assert_layers_equal(got, ref, f"device call on stream {stream}")
    multi = hb.HipScene(sc, devices=[0, 0])
    assert_layers_equal(multi.render_matte(cam, opts, id_kind="primitive", layers=8, residual=True), ref, "devices=[0, 0]")


def test_graph_of_layers_then_extraction_replays_the_eager_bytes(hb):
    """one stream, one chain of two kernels, captured as the first matte calls of any kind on a scene of its own; the eager bytes
    come from another scene object of the same description"""
    import torch
    sc, _, other, cam = _scene(hb, "all_materials")
    opts = _opts(W, H, SPP, 17)
    eager = other.render_matte(cam, opts, layers=4, residual=True)
    present = np.unique(eager["ids"][eager["coverage"] > 0])
    chosen = present[::2]  # ascending, as the device call wants it
    eager_matte = other.matte_extract(eager, None, chosen)
    assert 0 < eager_matte.max() and (eager_matte < 1).any()
    gpu = hb.HipScene(sc, device=0)
    dev = torch.device("cuda", 0)
    run = device_matte(torch, W, H, 4)
    selection = torch.from_numpy(chosen.view(np.int32).copy()).to(dev)  # (the same words: torch has no uint32 arithmetic to offer)

    def layers_then_extraction(stream):
        gpu.render_matte_device(cam, opts, run.ptrs(OUTPUTS), layers=4, stream=stream)
        gpu.matte_extract_device(run.ptr("ids"), run.ptr("coverage"), W, H, 4, selection.data_ptr(), len(chosen), run.ptr("matte"), stream=stream)

    g = capture(torch, layers_then_extraction)
    assert all(run.untouched(name) for name in run.buf)  # capture ran nothing
    g.replay()
    torch.cuda.synchronize(dev)
    for name in OUTPUTS:
        assert_same_bits(run.read(name), eager[name], f"graph replay {name}", nan_equal=False)
    assert_same_bits(run.read("matte"), eager_matte, "graph replay matte", nan_equal=False)


def test_no_side_effects_on_render(hb):
    sc, cam_params = ssml_scene("overshadowed")
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    assert_render_unaffected(gpu, cam, lambda opts, img: gpu.matte_extract(gpu.render_matte(cam, opts, residual=True), None, [0, 1]))


# ---- extraction ----
def test_extraction_matches_the_checker(hb):
    sc, _, gpu, cam = _scene(hb, "all_materials")
    layers = gpu.render_matte(cam, _opts(W, H, SPP, 3), id_kind="material", layers=8, residual=True)
    ids, cov = layers["ids"], layers["coverage"]
    present = np.unique(ids[cov > 0])
    assert SKY in present and len(present) >= 4  # the sky is seen, and several materials
    objects = present[present != SKY]

    def both(selection):
        got = gpu.matte_extract(ids, cov, selection)
        assert_same_bits(got, M.extract(ids, cov, selection), f"selection {np.asarray(selection).tolist()[:8]}", nan_equal=False)
        return got

    assert (both([]) == 0).all() and not np.signbit(both([])).any()
    one = both([int(objects[0])])
    assert 0 < one.max() <= 1 and (one == 0).any()
    sky = both([SKY])
    assert_same_bits(sky, np.where(ids == SKY, cov, F32(0)).sum(axis=0, dtype=F32), "the sky alone: empty layers must not match", nan_equal=False)
    everything = both(present)
    assert_same_bits(everything, (F32(1.0) - layers["residual"]).astype(np.float32), "every ID present: 1 - residual, exact in sixteenths", nan_equal=False)
    half = objects[: len(objects) // 2]
    rest = np.setdiff1d(present, half)
    assert_same_bits((both(half) + both(rest)).astype(np.float32), everything, "complementary selections", nan_equal=False)
    shuffled = np.concatenate([present[::-1], present, objects[:2]])  # unsorted, with duplicates: the host call sorts a copy
    assert_same_bits(both(shuffled), everything, "an unsorted selection with duplicates", nan_equal=False)
    absent = both([int(objects.max()) + 1, 0x7FFFFFFF])
    assert (absent == 0).all()


def test_a_selection_larger_than_the_staged_one(hb):
    """5000 IDs against the primitive layers of the mesh: past the 2048 a workgroup stages in LDS, so the search reads global memory"""
    _, _, gpu, cam = _scene(hb, "mesh2000_wide")
    layers = gpu.render_matte(cam, _opts(W, H, SPP, 3), id_kind="primitive", layers=8)
    ids, cov = layers["ids"], layers["coverage"]
    rng = np.random.default_rng(5)
    selection = rng.integers(0, 2000, 5000).astype(np.uint32)  # with duplicates; about 92 % of the primitives
    selection[::50] = rng.integers(2000, 1 << 32, 100).astype(np.uint32)  # and IDs that nothing has
    for sel in (selection, selection[:2048], selection[:2049]):  # both kernels, and both sides of the threshold
        got = gpu.matte_extract(ids, cov, sel)
        assert_same_bits(got, M.extract(ids, cov, sel), f"{len(sel)} IDs", nan_equal=False)
    assert 0 < (got > 0).mean() and (got < 1).any()


def test_full_frame_through_both_kernels(hb, O):
    sc, cam_params = ssml_scene("rtweekend1")
    gpu, cpu = hb.HipScene(sc, device=0), O.Scene(sc)
    cam, cam_c = hb.camera_new(**cam_params), O.camera_new(**cam_params)
    w, h, spp, k = 1920, 1080, 4, 4
    layers = gpu.render_matte(cam, _opts(w, h, spp, 1), id_kind="primitive", layers=k, residual=True)
    tiles_x, tiles_y = w // 8, h // 8
    rng = np.random.default_rng(0)
    tiles = {(0, 0), (tiles_x - 1, tiles_y - 1), (0, tiles_y - 1), (tiles_x - 1, 0)}
    while len(tiles) < 12:
        tiles.add((int(rng.integers(0, tiles_x)), int(rng.integers(0, tiles_y))))
    pixels = K.tile_pixels(w, h, sorted(tiles))
    ref = M.layers_from_pass_ids(M.pass_ids(sc, cpu, cam_c, w, h, spp, 1, 0, "primitive", pixels=pixels), k)
    assert_same_bits(layers["ids"].reshape(k, -1)[:, pixels], ref[0], "1080p tiles ids", nan_equal=False)
    assert_same_bits(layers["coverage"].reshape(k, -1)[:, pixels], ref[1], "1080p tiles coverage", nan_equal=False)
    assert_same_bits(layers["residual"].reshape(-1)[pixels], ref[2], "1080p tiles residual", nan_equal=False)
    n_prims = gpu.counts()[1]
    assert ((layers["ids"] < n_prims) | (layers["ids"] == SKY)).all()
    total = layers["residual"] + layers["coverage"].sum(axis=0, dtype=F32)
    assert (total == F32(1.0)).all()  # four passes: quarters
    selection = [0, SKY]  # the ground sphere and the sky
    matte = gpu.matte_extract(layers["ids"], layers["coverage"], selection)
    assert_same_bits(matte.reshape(-1)[pixels], M.extract(ref[0], ref[1], selection), "1080p tiles matte", nan_equal=False)
    whole = M.extract(layers["ids"], layers["coverage"], selection)
    assert_same_bits(matte, whole, "1080p matte against the checker on the library's layers", nan_equal=False)
    assert 0 < matte.mean() < 1
