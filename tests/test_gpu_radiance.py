"""Radiance queries (rt_radiance) on the GPU against the CPU oracle's fixed-ray integrator (tests/radiance_checker.py).  The
oracle runs on the streams (seed, 0, k), so every comparison with it queries with streams = 0 and one sample a ray at
sample_begin = k; the f64 prefix means of the GPU's samples must then EQUAL the oracle's.  GPU against GPU, every comparison is
bit-exact (NaN == NaN).  An oracle result is computed once per (scene, ray set, options) and shared."""
import functools

import numpy as np
import pytest

import aov_checker as K
import hard_tree_cases as HT
import radiance_checker as R
import scenes
from gpu_support import assert_render_unaffected, assert_same_bits, capture, radiance_device_run, ssml_scene

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
GW, GH, SEED, NK = 32, 18, 5, 4
METHODS = (abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS)

SCENES = {
    "emit_scene": lambda: (K.emit_scene(), K.EMIT_CAMERA),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "spheres500": lambda: (scenes.random_spheres(500, emissive_every=10), scenes.ALL_MATERIALS_CAMERA),
    "pyramid": lambda: ssml_scene("pyramid"),
    "rtweekend1": lambda: ssml_scene("rtweekend1"),
    "overshadowed": lambda: ssml_scene("overshadowed"),
    "mesh2000": lambda: (scenes.random_triangle_mesh(2000, edge=2.0), scenes.MESH_CAMERA),
    "mesh20000": lambda: (scenes.random_triangle_mesh(20000, edge=1.0), scenes.MESH_CAMERA),
}
BOUNCING = ("all_materials", "rtweekend1", "spheres500", "mesh2000")


@functools.lru_cache(maxsize=None)
def _built(name):
    """(scene description, camera parameters, oracle scene, oracle camera), once per scene; hard trees by their case name"""
    import oracle as O
    O.build()
    if name in SCENES:
        sc, cam_params = SCENES[name]()
        return sc, cam_params, O.Scene(sc), O.camera_new(**cam_params)
    return HT.built(name)


@functools.lru_cache(maxsize=None)
def _rays(name, which, w=GW, h=GH):
    """ray set "a": the camera's rays through the pixel centres of a w x h grid; "b": surface probes from the hits of (a)"""
    _, _, cpu, cam = _built(name)
    o, d = R.pixel_centre_rays(cam, w, h)
    if which == "b":
        o, d = R.surface_probes(cpu, o, d, seed=11)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def _degenerate_rays():
    o, d = [], []
    for direction in ((0, 0, 0), (np.nan, 0, -1), (0, np.nan, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        o.append((0.0, 1.5, 6.0))
        d.append(direction)
    for direction in ((0, -1, 0), (0, 0, -1), (1, 0, 0)):  # axis-parallel, from above the balls and along their row
        o.append((0.0, 3.5, 0.0) if direction[1] else (-4.0, 0.5, 0.0) if direction[0] else (1.1, 0.5, 5.0))
        d.append(direction)
    for direction in ((0.3, 0.2, -1.0), (0, 1, 0), (-1, -0.1, 0.2), (0, 0, 0)):  # from inside the glass sphere
        o.append((0.0, 0.5, 0.0))
        d.append(direction)
    for direction in ((-1, -1, -1), (1, 0, 0), (0.1, -0.2, 0.3)):  # from 1e30 away
        o.append((1e30, 1e30, 1e30))
        d.append(direction)
    o.append((np.inf, 0.0, 0.0))
    d.append((-1, 0, 0))
    return np.array(o, dtype=F32), np.array(d, dtype=F32)


@functools.lru_cache(maxsize=None)
def _ray_set(name, which, n=None):
    if which == "degenerate":
        return _degenerate_rays()
    if which == "repeat":  # n rays: set (a) and then set (b), over and over
        a, b = _rays(name, "a"), _rays(name, "b")
        o, d = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
        idx = np.arange(n) % len(o)
        return o[idx], d[idx]
    o, d = _rays(name, which)
    return (o, d) if n is None else (o[:n], d[:n])


@functools.lru_cache(maxsize=None)
def _oracle(name, which, n, method, k, seed, max_depth=50, rr_threshold=3):
    """[rays, k, 3] f64 prefix means"""
    _, _, cpu, _ = _built(name)
    o, d = _ray_set(name, which, n)
    r = R.prefix_means(cpu, o, d, method, k, seed=seed, max_depth=max_depth, rr_threshold=rr_threshold)
    r.setflags(write=False)
    return r


def _gpu(hb, name, **kw):
    sc, cam_params, _, _ = _built(name)
    return hb.HipScene(sc, **(kw or dict(device=0))), hb.camera_new(**cam_params)


def _samples(gpu, o, d, method, k, seed, **kw):
    """[n, k, 3] f32: sample j of every ray on stream 0, one query a sample"""
    return R.samples(gpu, o, d, method, k, seed, **kw)


def _assert_matches_oracle(gpu, name, which, n, method, k, seed, what, **kw):
    o, d = _ray_set(name, which, n)
    return R.assert_matches(gpu, o, d, _oracle(name, which, n, method, k, seed, **kw), method, seed, what, **kw)


# ---- per-sample parity ----
@pytest.mark.parametrize("name", list(SCENES))
def test_samples_match_the_oracle(hb, name):
    gpu, _ = _gpu(hb, name)
    for which in ("a", "b"):
        o, d = _ray_set(name, which)
        assert len(o) >= (GW * GH if which == "a" else 50), (name, which, len(o))
        for method in METHODS:
            ref = _oracle(name, which, None, method, NK, SEED)
            assert np.isfinite(ref).all(), (name, which, method)
            if which == "a":
                bounced = float((ref[:, 0] != ref[:, 1]).any(axis=1).mean())
                lit = float((ref[:, NK - 1] != 0.0).any(axis=1).mean())
                print(f"{name} method {method}: sample 0 != sample 1 on {bounced:.3f} of the rays, non-zero mean on {lit:.3f}")
                if name in BOUNCING:  # the paths really bounced and drew
                    assert bounced >= 0.25, (name, method, bounced)
                if name == "overshadowed" and method == abi.RT_METHOD_MIS:  # the emissive-primitive check_hit_index arm
                    assert lit >= 0.9, lit
            first = None
            for mode in (0, 1, -1):  # forced exhaustive / pruned, automatic: the same bytes
                gpu.set_traversal(mode)
                got = _samples(gpu, o, d, method, NK, SEED)
                if first is None:
                    first = got
                    R.assert_same_f64(R.fold_prefix(got), ref, f"{name} set {which} method {method}")
                else:
                    assert_same_bits(got, first, f"{name} set {which} method {method} traversal {mode}", nan_equal=True)


def test_the_wide_walk_and_the_two_child_walk_give_the_same_bytes(hb):
    name = "mesh20000"
    gpu, _ = _gpu(hb, name)
    assert len(gpu.wide_tree()[0]) > 0, "the scene has no wide tree: the case tests nothing"
    gpu.set_traversal(1)
    o, d = _ray_set(name, "b")
    for method in METHODS:
        ref = _oracle(name, "b", None, method, NK, SEED)
        for walk in (0, 1):
            gpu.set_tuning(abi.RT_TUNE_WALK, walk)
            R.assert_same_f64(R.fold_prefix(_samples(gpu, o, d, method, NK, SEED)), ref, f"walk {walk} method {method}")


# ---- the summation rule ----
def test_five_samples_from_sample_three_fold_by_the_rule(hb):
    name = "all_materials"
    gpu, _ = _gpu(hb, name)
    o, d = _ray_set(name, "repeat", 257)
    for method in METHODS:
        for streams in (None, np.zeros(len(o), dtype=np.uint64)):
            singles = np.stack([gpu.radiance(o, d, streams=streams, method=method, samples=1, seed=9, sample_begin=j) for j in range(3, 8)], axis=1)
            got = gpu.radiance(o, d, streams=streams, method=method, samples=5, seed=9, sample_begin=3)
            assert_same_bits(got, R.fold_f32(singles), f"method {method}: K = 5 from sample 3", nan_equal=True)
            assert (singles[:, 0] != singles[:, 1]).any()
        one = gpu.radiance(o, d, method=method, samples=1, seed=9, sample_begin=3)
        assert_same_bits(one, R.fold_f32(one[:, None, :]), "K = 1 is the sample", nan_equal=True)


# ---- streams ----
def test_streams(hb):
    name = "spheres500"
    gpu, _ = _gpu(hb, name)
    o, d = _ray_set(name, "repeat", 300)
    n = len(o)
    for method in METHODS:
        kw = dict(method=method, samples=2, seed=4)
        base = gpu.radiance(o, d, **kw)
        assert_same_bits(gpu.radiance(o, d, streams=np.arange(n, dtype=np.uint64), **kw), base, "NULL streams are 0 .. n-1", nan_equal=True)
        perm = np.random.default_rng(2).permutation(n)
        assert_same_bits(gpu.radiance(o[perm], d[perm], streams=perm.astype(np.uint64), **kw), base[perm], "rays permuted with their streams",
                         nan_equal=True)
        # equal origin, direction and stream: equal rows; another stream: another row somewhere
        probe = int(np.argmax((base != 0).any(axis=1) & (gpu.radiance(o, d, streams=np.full(n, 7, np.uint64), **kw) != base).any(axis=1)))
        oo, dd = np.repeat(o[probe][None], 64, axis=0), np.repeat(d[probe][None], 64, axis=0)
        st = np.array([3, 3] + list(range(1 << 40, (1 << 40) + 62)), dtype=np.uint64)
        rows = gpu.radiance(oo, dd, streams=st, **kw)
        assert_same_bits(rows[0], rows[1], "equal ray, equal stream", nan_equal=True)
        assert len({r.tobytes() for r in rows[1:]}) > 8, "different streams give the same rows"


# ---- shapes and the refill ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_batch_sizes(hb, n):
    name = "all_materials"
    gpu, _ = _gpu(hb, name)
    for method in METHODS:
        got = _assert_matches_oracle(gpu, name, "repeat", n, method, 2, SEED, f"n = {n} method {method}")
        if n == 1000:  # one workgroup: every lane works through four rays, and through their samples in order
            o, d = _ray_set(name, "repeat", n)
            gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, 1)
            capped = _assert_matches_oracle(gpu, name, "repeat", n, method, 2, SEED, f"n = {n} method {method}, one workgroup")
            assert_same_bits(capped, got, "one workgroup against the automatic launch", nan_equal=True)
            k3 = gpu.radiance(o, d, method=method, samples=3, seed=8)
            gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, 0)
            assert_same_bits(gpu.radiance(o, d, method=method, samples=3, seed=8), k3, "three samples a ray, one workgroup or many", nan_equal=True)


# ---- options ----
@pytest.mark.parametrize("max_depth", [1, 2, 8, 50])
@pytest.mark.parametrize("rr_threshold", [0, 3])
def test_max_depth_and_rr_threshold(hb, max_depth, rr_threshold):
    name = "all_materials"
    gpu, _ = _gpu(hb, name)
    for method in METHODS:
        _assert_matches_oracle(gpu, name, "repeat", 257, method, 2, SEED, f"max_depth {max_depth} rr {rr_threshold} method {method}",
                               max_depth=max_depth, rr_threshold=rr_threshold)


# ---- degenerate rays and hard trees ----
def test_degenerate_rays(hb):
    name = "all_materials"
    gpu, _ = _gpu(hb, name)
    for method in METHODS:
        for mode in (0, 1):
            gpu.set_traversal(mode)
            _assert_matches_oracle(gpu, name, "degenerate", None, method, NK, SEED, f"degenerate rays method {method} traversal {mode}")


HARD = ["single_sphere"] + [c for c in HT.CASES if c.startswith(("spheres2_", "triangles2_"))] + ["non_finite_geometry"]


@pytest.mark.parametrize("case", HARD)
def test_hard_trees(hb, case):
    gpu, _ = _gpu(hb, case)
    for method in METHODS:
        for mode in (0, 1):
            gpu.set_traversal(mode)
            _assert_matches_oracle(gpu, case, "a", 64, method, 2, SEED, f"{case} method {method} traversal {mode}")


# ---- entry points ----
def _device_run(torch, gpu, o, d, streams, off, stream=0, **kw):
    return radiance_device_run(torch, gpu, o, d, streams, off, **kw)


def test_host_entry_device_entry_alignment_streams_and_a_multi_device_head(hb):
    import torch
    name = "all_materials"
    o, d = _ray_set(name, "repeat", 257)
    streams = (np.arange(257, dtype=np.uint64) * 3) % 17
    dev = torch.device("cuda", 0)
    for what, kw in (("device=0", dict(device=0)), ("devices=[0, 0]", dict(devices=[0, 0]))):
        gpu, _ = _gpu(hb, name, **kw)
        for method in METHODS:
            opts = dict(method=method, samples=2, seed=6, sample_begin=1)
            ref = gpu.radiance(o, d, streams=streams, **opts)
            if method == abi.RT_METHOD_MIS:
                zeros = gpu.radiance(o, d, streams=np.zeros(257, np.uint64), method=method, samples=1, seed=SEED)
                R.assert_same_f64(R.fold_prefix(zeros[:, None, :]), _oracle(name, "repeat", 257, method, 2, SEED)[:, :1], f"{what} host entry")
            created = torch.cuda.Stream(device=dev)
            for off in (0, 1, 3):  # 0, 4 and 12 bytes off a 16-byte boundary
                for stream in (0, created.cuda_stream):
                    bufs, enqueue, keep = _device_run(torch, gpu, o, d, streams, off, **opts)
                    torch.cuda.synchronize()
                    enqueue(stream)
                    torch.cuda.synchronize()
                    assert_same_bits(bufs.read("out"), ref, f"{what} device entry off {off} stream {stream != 0}", nan_equal=True)
                    assert bufs.read("rays").tobytes() == np.concatenate([o, d], axis=1).astype(F32).tobytes()
    # n = 0: nothing is written
    bufs, enqueue, keep = _device_run(torch, gpu, o, d, None, 0)
    gpu.radiance_device(bufs.ptr("rays"), 0, 0, bufs.ptr("out"))
    torch.cuda.synchronize()
    assert bufs.untouched("out")
    assert gpu.radiance(o[:0], d[:0]).shape == (0, 3)


def test_three_streams_in_flight_twice_over(hb):
    import torch
    name = "all_materials"
    gpu, _ = _gpu(hb, name)
    o, d = _ray_set(name, "repeat", 1000)
    opts = dict(method=abi.RT_METHOD_MIS, samples=2, seed=6)
    ref = gpu.radiance(o, d, **opts)
    gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, 2)  # the launches overlap and every lane refills
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    runs = [_device_run(torch, gpu, o, d, None, 0, **opts) for _ in streams]
    torch.cuda.synchronize()
    for _ in range(2):
        for s, (bufs, enqueue, keep) in zip(streams, runs):  # in flight together
            enqueue(s.cuda_stream)
    torch.cuda.synchronize()
    for i, (bufs, enqueue, keep) in enumerate(runs):
        assert_same_bits(bufs.read("out"), ref, f"stream {i}", nan_equal=True)


def test_graph_captured_from_the_first_call_replays_the_same_bytes(hb):
    """no warm-up: the first query of a fresh scene is the captured one"""
    import torch
    name = "all_materials"
    o, d = _ray_set(name, "repeat", 1000)
    opts = dict(method=abi.RT_METHOD_MIS, samples=2, seed=6)
    fresh, _ = _gpu(hb, name)
    bufs, enqueue, keep = _device_run(torch, fresh, o, d, None, 0, **opts)
    g = capture(torch, enqueue)
    assert bufs.untouched("out")  # capture ran nothing
    other, _ = _gpu(hb, name)
    ref = other.radiance(o, d, **opts)
    dev = torch.device("cuda", 0)
    for _ in range(2):
        bufs.buf["out"].fill_(bufs.guard)
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        assert_same_bits(bufs.read("out"), ref, "graph replay", nan_equal=True)


def test_no_side_effects_on_render(hb):
    gpu, cam = _gpu(hb, "overshadowed")
    o, d = _ray_set("overshadowed", "a")
    assert_render_unaffected(gpu, cam, lambda opts, img: gpu.radiance(o, d, samples=2))


# ---- full size ----
def test_a_1080p_grid_of_rays(hb):
    name = "all_materials"
    _, _, cpu, cam = _built(name)
    gpu, _ = _gpu(hb, name)
    w, h = 1920, 1080
    o, d = R.pixel_centre_rays(cam, w, h)
    zeros = np.zeros(w * h, dtype=np.uint64)
    got = gpu.radiance(o, d, streams=zeros, method=abi.RT_METHOD_MIS, samples=1, seed=SEED)
    pick = np.unique(np.concatenate([np.arange(64), np.arange(w * h - 64, w * h), np.sort(np.random.default_rng(0).choice(w * h, 4096, replace=False))]))
    ref = R.prefix_means(cpu, o[pick], d[pick], abi.RT_METHOD_MIS, 1, seed=SEED)
    R.assert_same_f64(R.fold_prefix(got[pick][:, None, :]), ref, "1080p subset")
    assert np.isfinite(ref).all() and np.isfinite(got[pick]).all()
    assert (got[pick] != 0).any()
