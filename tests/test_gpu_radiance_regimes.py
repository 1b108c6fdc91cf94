"""Radiance queries (rt_radiance) on the inputs of tests/radiance_cases.py: every hard tree (the chain: 87 040 B of dynamic LDS a
workgroup), every sky regime through this kernel's own sample_lights / pdf_from_index, the four arms of sample_lights, and
streams, seeds and sample indices as 64-bit values.  test_radiance_cases.py (CPU) shows that each entry tests something.  Every
comparison is with the oracle -- the f64 prefix means of the GPU's samples EQUAL the oracle's -- or bit for bit GPU against GPU
(NaN == NaN).  There is no tolerance in this file."""
import numpy as np
import pytest

import radiance_cases as RC
import radiance_checker as R
import scenes
import sky_cases as SK
from gpu_support import assert_render_unaffected, assert_same_bits, capture, radiance_device_run

pytestmark = pytest.mark.gpu
abi = scenes.abi
SEED = RC.SEED


def _gpu(hb, key):
    sc, cam_params, _, _ = RC.built(key)
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


def _against_oracle(gpu, key, method, what, n=None):
    o, d = RC.rays(key)[:2] if n is None else RC.repeated(key, n)
    return R.assert_matches(gpu, o, d, RC.reference(key, method, n), method, SEED, f"{key} method {method} {what}")


# ---- hard trees ----
@pytest.mark.parametrize("key", RC.TREES)
def test_hard_tree(hb, key):
    gpu, _ = _gpu(hb, key)
    o, d, _ = RC.rays(key)
    k = RC.ENTRIES[key].k
    wide = len(gpu.wide_tree()[0]) > 0
    for method in RC.METHODS:
        gpu.set_traversal(0)
        first = _against_oracle(gpu, key, method, "traversal 0")
        for mode in (1, -1):
            gpu.set_traversal(mode)
            assert_same_bits(R.samples(gpu, o, d, method, k, SEED), first, f"{key} method {method} traversal {mode}", nan_equal=True)
        if wide:
            gpu.set_traversal(1)
            for walk in (0, 1):
                gpu.set_tuning(abi.RT_TUNE_WALK, walk)
                assert_same_bits(R.samples(gpu, o, d, method, k, SEED), first, f"{key} method {method} pruned, walk {walk}", nan_equal=True)
            gpu.set_tuning(abi.RT_TUNE_WALK, 0)
    if key == "tree/chain":
        assert wide and RC.four_wave_lds_bytes(gpu.wide_tree()[2]) == 87040


# ---- the chain: more than 64 KB of dynamic LDS a workgroup ----
CHAIN = "tree/chain"


def test_chain_one_workgroup_refills_under_87040_bytes_of_lds(hb):
    gpu, _ = _gpu(hb, CHAIN)
    o, d = RC.repeated(CHAIN, 300)
    for method in RC.METHODS:
        free = _against_oracle(gpu, CHAIN, method, "300 rays", n=300)
        k3 = gpu.radiance(o, d, method=method, samples=3, seed=8)
        gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, 1)  # 256 lanes, 300 rays: every wave takes a second block, lanes refill
        capped = _against_oracle(gpu, CHAIN, method, "300 rays, one workgroup", n=300)
        assert_same_bits(capped, free, f"method {method}: one workgroup against the automatic launch", nan_equal=True)
        assert_same_bits(gpu.radiance(o, d, method=method, samples=3, seed=8), k3, f"method {method}: three samples a ray", nan_equal=True)
        gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, 0)


def test_chain_device_entry_off_alignment(hb):
    import torch
    gpu, _ = _gpu(hb, CHAIN)
    o, d = RC.repeated(CHAIN, 300)
    streams = (np.arange(300, dtype=np.uint64) * 3) % 17
    for method in RC.METHODS:
        opts = dict(method=method, samples=2, seed=6, sample_begin=1)
        ref = gpu.radiance(o, d, streams=streams, **opts)
        for off in (0, 1, 3):  # 0, 4 and 12 bytes off a 16-byte boundary
            bufs, enqueue, keep = radiance_device_run(torch, gpu, o, d, streams, off, **opts)
            torch.cuda.synchronize()
            enqueue(0)
            torch.cuda.synchronize()
            assert_same_bits(bufs.read("out"), ref, f"method {method} device entry off {off}", nan_equal=True)
            assert bufs.read("rays").tobytes() == np.concatenate([o, d], axis=1).astype(np.float32).tobytes()


def test_chain_graph_captured_from_the_first_call_replays_the_same_bytes(hb):
    """no warm-up: the first query of a fresh chain scene is the captured one (hipFuncSetAttribute for 87 040 B under capture)"""
    import torch
    o, d = RC.repeated(CHAIN, 300)
    opts = dict(method=abi.RT_METHOD_MIS, samples=2, seed=6)
    fresh, _ = _gpu(hb, CHAIN)
    bufs, enqueue, keep = radiance_device_run(torch, fresh, o, d, None, 0, **opts)
    g = capture(torch, enqueue)
    assert bufs.untouched("out")  # capture ran nothing
    other, _ = _gpu(hb, CHAIN)
    ref = other.radiance(o, d, **opts)
    dev = torch.device("cuda", 0)
    for _ in range(2):
        bufs.buf["out"].fill_(bufs.guard)
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        assert_same_bits(bufs.read("out"), ref, "graph replay", nan_equal=True)


def test_chain_query_has_no_side_effects_on_render(hb):
    gpu, cam = _gpu(hb, CHAIN)
    o, d, _ = RC.rays(CHAIN)
    assert_render_unaffected(gpu, cam, lambda opts, img: gpu.radiance(o, d, samples=2))


# ---- sky regimes through this kernel's sample_lights and pdf_from_index ----
@pytest.mark.parametrize("key", RC.SKIES)
def test_sky_regime(hb, key):
    _, case, scene = key.split("/")
    gpu, _ = _gpu(hb, key)
    si = gpu.sky_info()
    assert (si["guide_k"], si["inv_res_ok"]) == (SK.CASES[case].guide_k, SK.CASES[case].inv_res_ok)
    o, d, _ = RC.rays(key)
    k = RC.ENTRIES[key].k
    naive = None
    for method in RC.METHODS:
        for mode in (0, 1):
            gpu.set_traversal(mode)
            got = _against_oracle(gpu, key, method, f"traversal {mode}")
            if method == RC.NAIVE:
                naive = got
    # NAIVE never samples the sky: the same bytes with no sampler at all
    plain = hb.HipScene(RC.unsampled_scene(case, scene), device=0)
    assert plain.sky_info()["res_x"] == 0 and plain.sky_info()["res_y"] == 0
    plain.set_traversal(1)
    assert_same_bits(R.samples(plain, o, d, RC.NAIVE, k, SEED), naive, f"{key}: NAIVE under the sampled sky and under sampler_res (0, 0)",
                     nan_equal=True)


# ---- the four arms of sample_lights ----
@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_sample_lights_shape(hb, name):
    key = f"shape/{name}"
    gpu, _ = _gpu(hb, key)
    si = gpu.sky_info()
    assert (gpu.counts()[2] > 0, (si["res_x"] | si["res_y"]) != 0) == RC.SHAPES[name][0]
    assert RC.reference(key, RC.MIS).shape[1] == 4
    _against_oracle(gpu, key, RC.MIS, "K = 4")


# ---- streams, seeds and sample indices as 64-bit values ----
@pytest.mark.parametrize("seed", RC.SEEDS)
@pytest.mark.parametrize("method", RC.METHODS)
def test_streams_seeds_and_sample_indices_against_the_oracle(hb, method, seed):
    import torch
    key = "streams"
    gpu, _ = _gpu(hb, key)
    o, d, _ = RC.rays(key)
    st = RC.streams()
    for begin in RC.SAMPLE_BEGINS:
        what = f"method {method} seed {seed:#x} sample_begin {begin:#x}"
        singles = R.assert_matches(gpu, o, d, RC.stream_reference(method, seed, begin), method, seed, what, streams=st, sample_begin=begin)
        if begin in ((1 << 32) - 1, (1 << 64) - 2):  # K = 3 in ONE query: the carry into the high word, and the wrap, in the kernel's own sum
            opts = dict(method=method, samples=RC.STREAM_K, seed=seed, sample_begin=begin)
            folded = R.fold_f32(singles)
            assert_same_bits(gpu.radiance(o, d, streams=st, **opts), folded, f"{what}: three samples, host entry", nan_equal=True)
            bufs, enqueue, keep = radiance_device_run(torch, gpu, o, d, st, 0, **opts)
            torch.cuda.synchronize()
            enqueue(0)
            torch.cuda.synchronize()
            assert_same_bits(bufs.read("out"), folded, f"{what}: three samples, device entry", nan_equal=True)
    if seed == RC.SEEDS[0]:  # the device entry reads the same 64-bit streams from a device array, one sample a query
        ref = RC.stream_reference(method, seed, 0)
        bufs, enqueue, keep = radiance_device_run(torch, gpu, o, d, st, 1, method=method, samples=1, seed=seed, sample_begin=0)
        torch.cuda.synchronize()
        enqueue(0)
        torch.cuda.synchronize()
        R.assert_same_f64(R.fold_prefix(bufs.read("out")[:, None, :]), ref[:, :1], f"method {method}: device entry, one sample")
