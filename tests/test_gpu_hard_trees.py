"""The four tile kernels (rt_render_aov, rt_render_aov_chain, rt_render_matte, rt_render_ao) on the trees built to break walks
(tests/hard_tree_cases.py; test_hard_trees.py shows on the CPU that every case tests something): every channel bit for bit
against the stage's checker under every traversal mode and both walks.  On the chain scene, whose four-wave stacks take 87 040
bytes of LDS, also the device entries into guarded buffers, a graph captured as the scene's first launch, and the render around
all four stages."""
import functools

import numpy as np
import pytest

import hard_tree_cases as HT
import matte_checker as M
import scenes
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture

pytestmark = pytest.mark.gpu
abi = scenes.abi
W, H = HT.W, HT.H
SKY = abi.AOV_NO_ID
PAIRS = [(stage, name) for stage in HT.STAGES for name in HT.CASES]  # a stage at a time, the chain scene last


def _opts():
    return abi.default_render_opts(W, H, HT.SPP, seed=HT.SEED)


def _gpu(hb, name):
    sc, cam_params, _, _ = HT.built(name)
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


@functools.lru_cache(maxsize=None)
def _reference(name, stage, radius=0.0):
    """the checker's channels as the host entry shapes them, once per (case, stage, options)"""
    if stage == "aov":
        return HT.framed(HT.aov(name))
    if stage == "aov_chain":
        return HT.framed(HT.aov_chain(name))
    if stage == "ao":
        r = HT.ao(name, radius)
        return HT.framed({k: r[k] for k in abi.AO_CHANNELS})
    ids, coverage, residual = HT.matte(name)["primitive"]
    k = HT.MATTE_LAYERS
    return {"ids": ids.reshape(k, H, W), "coverage": coverage.reshape(k, H, W), "residual": residual.reshape(H, W)}


def _host_entry(gpu, cam, stage, radius=0.0):
    if stage == "aov":
        return gpu.render_aov(cam, _opts())
    if stage == "aov_chain":
        return gpu.render_aov_chain(cam, _opts())
    if stage == "ao":
        return gpu.render_ao(cam, _opts(), rays_per_pass=HT.RAYS, radius=radius)
    return gpu.render_matte(cam, _opts(), id_kind="primitive", layers=HT.MATTE_LAYERS, residual=True)


def _device_entry(gpu, cam, stage, ptrs, stream=0):
    if stage == "aov":
        gpu.render_aov_device(cam, _opts(), ptrs, stream=stream)
    elif stage == "aov_chain":
        gpu.render_aov_chain_device(cam, _opts(), ptrs, stream=stream)
    elif stage == "ao":
        gpu.render_ao_device(cam, _opts(), ptrs, rays_per_pass=HT.RAYS, stream=stream)
    else:
        gpu.render_matte_device(cam, _opts(), ptrs, id_kind="primitive", layers=HT.MATTE_LAYERS, stream=stream)


def _buffers(torch, stage, ref, off=0):
    """guarded device buffers shaped like the host entry's result; the matte's guard is a NaN pattern, which its strict compare
    tells from any output, the other stages' is an ordinary number, which their NaN-tolerant compare does"""
    guard = 0x7FC0BEEF if stage == "matte" else 0x5A5A5A5A
    return GuardedBuffers(torch, {name: (a.shape, a.dtype.type) for name, a in ref.items()}, off=off, guard=guard)


def assert_stage_equal(got, ref, stage, what):
    """the matte's planes compare strictly (its guard and nothing it writes is a NaN); elsewhere any NaN equals any NaN"""
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for name in ref:
        if stage == "matte":
            assert_same_bits(got[name], ref[name], f"{what} {name}", nan_equal=False)
        else:
            assert_same_bits(got[name], ref[name], f"{what} {name}", nan_equal=True)


def _radii(name, stage):
    case = HT.CASES[name]
    return (0.0, case.radius) if stage == "ao" and case.radius else (0.0,)


@pytest.mark.parametrize("stage,name", PAIRS, ids=[f"{stage}.{name}" for stage, name in PAIRS])
def test_hard_tree(hb, stage, name):
    gpu, cam = _gpu(hb, name)
    case = HT.CASES[name]
    if stage == "ao" and case.radius:  # the finite radius opens rays the unlimited one finds occluded
        assert (HT.ao(name, case.radius)["open"] & ~HT.ao(name, 0.0)["open"]).any()
    try:
        for mode in (0, 1, -1):  # forced exhaustive / pruned, automatic: the same bytes
            gpu.set_traversal(mode)
            for walk in ((0, 1) if mode == 1 else (0,)):  # the wide tree where the scene has one / the two-child tree for every ray
                gpu.set_tuning(abi.RT_TUNE_WALK, walk)
                for radius in _radii(name, stage):
                    got = _host_entry(gpu, cam, stage, radius)
                    assert_stage_equal(got, _reference(name, stage, radius), stage, f"{name} {stage} traversal={mode} walk={walk} radius={radius}")
        if stage == "matte":
            ref = _reference(name, stage)
            present = np.unique(ref["ids"][(ref["coverage"] > 0) & (ref["ids"] != SKY)])
            selection = [int(present[0]), int(SKY)]
            matte = gpu.matte_extract(got["ids"], got["coverage"], selection)
            assert_same_bits(matte, M.extract(ref["ids"], ref["coverage"], selection), f"{name} matte of {selection}", nan_equal=False)
            assert matte.max() > 0
    finally:
        gpu.set_tuning(abi.RT_TUNE_WALK, 0)
        gpu.set_traversal(-1)


# ---- the chain scene: 85 stack entries x 4 waves x 256 B = 87 040 B of dynamic LDS ----
@pytest.mark.parametrize("stage", HT.STAGES)
def test_chain_device_entry_off_alignment_with_guards(hb, stage):
    import torch
    gpu, cam = _gpu(hb, "chain")
    assert gpu.wide_tree()[2] * 1024 > 65536
    host = _host_entry(gpu, cam, stage)
    assert_stage_equal(host, _reference("chain", stage), stage, f"chain {stage} host entry")
    for off in (1, 3):  # 4 and 12 bytes off a 16-byte boundary
        run = _buffers(torch, stage, host, off)
        torch.cuda.synchronize()
        _device_entry(gpu, cam, stage, run.ptrs())
        torch.cuda.synchronize()
        assert_stage_equal(run.read_all(), host, stage, f"chain {stage} device entry off={off}")  # (read() checks the guard words)


@pytest.mark.parametrize("stage", HT.STAGES)
def test_chain_graph_captured_as_the_first_launch(hb, stage):
    """a scene object that has launched nothing: the captured call is the one that raises the kernel's dynamic LDS limit"""
    import torch
    eager_scene, cam = _gpu(hb, "chain")
    eager = _host_entry(eager_scene, cam, stage)
    gpu, cam = _gpu(hb, "chain")
    dev = torch.device("cuda", 0)
    run = _buffers(torch, stage, eager)
    g = capture(torch, lambda stream: _device_entry(gpu, cam, stage, run.ptrs(), stream=stream))
    assert all(run.untouched(name) for name in run.buf)  # capture ran nothing
    for _ in range(2):
        run.refill()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        assert_stage_equal(run.read_all(), eager, stage, f"chain {stage} graph replay")


def test_no_side_effects_on_render(hb):
    gpu, cam = _gpu(hb, "chain")

    def all_four(opts, img):
        gpu.render_aov(cam, opts)
        gpu.render_aov_chain(cam, opts)
        gpu.matte_extract(gpu.render_matte(cam, opts, id_kind="primitive", residual=True), None, [0, SKY])
        gpu.render_ao(cam, opts, rays_per_pass=HT.RAYS)

    assert_render_unaffected(gpu, cam, all_four)
