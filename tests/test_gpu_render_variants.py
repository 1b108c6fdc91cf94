"""render_kernel's variants on the trees built to break walks (tests/render_variant_cases.py; test_render_variant_cases.py shows on
the CPU that no entry is vacuous): every case under both integrators, three work shapes (sample_split 1 and 2, shard 1 of 3
packed) and every variant of the table -- traversal, schedule, walk, scene in LDS, exchange, feature set, forced stack cap --
bit for bit against the CPU oracle's frame, the ray count equal, and rt_last_launch_info equal to the launch the table derives
from the header's rules.  The chain seen along its axis, whose walks leave 84 entries pending, also through rt_render_device
into guarded buffers off alignment."""
import numpy as np
import pytest

import render_variant_cases as RV
import scenes
from gpu_support import GuardedBuffers, assert_same_bits

pytestmark = pytest.mark.gpu
abi = scenes.abi


def _apply(gpu, v):
    for field, key in RV.KEYS.items():
        value = getattr(v, field)
        if value is not None:  # (no feature set named: the library's own)
            gpu.set_tuning(key, value)


def _reset(gpu):
    """back to automatic (a named feature set stays named: the scene is not used again)"""
    _apply(gpu, RV.AUTOMATIC)


def _launch(info):
    return RV.Launch(info["fine"], info["pruned"], info["scene_in_lds"], info["feature_set"], info["kernel"].endswith(", true>"))


def _gpu(hb, name):
    sc, cam_params, _, _ = RV.built(name)
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


@pytest.mark.parametrize("name", RV.CASES)
def test_render_variants(hb, name):
    gpu, cam = _gpu(hb, name)
    f = RV.facts(name)
    assert (len(gpu.wide_tree()[0]) > 0) == f.wide
    run, refused = RV.variants_for(name)
    renders = 0
    try:
        # the shard under automatic settings, checked once against the oracle's frame: its ray count is the variants' reference
        shard_rays = {}
        for method in RV.METHODS:
            img, rays = gpu.render(cam, RV.options(method, "shard1of3"))
            assert_same_bits(img, RV.reference(name, method, "shard1of3")[0], f"{name} m={method} shard, automatic", nan_equal=True)
            assert rays == RV.oracle_shard_rays(name, method)
            shard_rays[method] = rays
        for fs in refused:  # a feature set below the scene's own is refused, not run
            with pytest.raises(hb.RtHipError):
                gpu.set_tuning(abi.RT_TUNE_FEATURE_SET, fs)
        for v in run:
            _apply(gpu, v)
            for method in RV.METHODS:
                want = RV.expected_launch(name, v, method)
                for shape in RV.SHAPES:
                    what = RV.describe(name, method, shape, v)
                    img, rays = gpu.render(cam, RV.options(method, shape))
                    ref, ref_rays = RV.reference(name, method, shape)
                    assert_same_bits(img, ref, what, nan_equal=True)
                    assert rays == (shard_rays[method] if ref_rays is None else ref_rays), what
                    info = gpu.last_launch_info()
                    assert _launch(info) == want, (what, info)
                    assert info["sample_split"] == (1 if shape == "split1" else 2), (what, info)
                    if want.fine:  # the exchange's workgroups, and a forced cap that leaves the rest of the worst case outside LDS
                        assert info["block_threads"] == 512 or not want.exchange, (what, info)
                        depth = gpu.wide_tree()[2]
                        if v.stack_cap and v.stack_cap * 2 <= depth and depth >= 64:  # (the chain: stacks are most of the LDS)
                            assert info["lds_bytes"] < depth * info["block_threads"] * 4, (what, info)
                    renders += 1
    finally:
        _reset(gpu)
    assert renders == len(run) * len(RV.METHODS) * len(RV.SHAPES)


@pytest.mark.parametrize("name", ["chain", "chain_along_axis"])
def test_chain_device_entry_off_alignment_fine_exchange_forced_cap(hb, name):
    """rt_render_device under the fine schedule with the exchange on (512-thread workgroups, the pools behind the stacks) and the
    middle forced cap: frame and device ray counter between guard words, the frame 4 and 12 bytes off a 16-byte boundary"""
    import torch
    gpu, cam = _gpu(hb, name)
    v = RV.Variant(1, 1, 0, 1, 1, None, RV.MIDDLE_CAP)
    assert v in RV.VARIANTS
    try:
        _apply(gpu, v)
        for method in RV.METHODS:
            for shape in ("split1", "split2"):
                ref, ref_rays = RV.reference(name, method, shape)
                for off in (1, 3):
                    what = RV.describe(name, method, shape, v) + f" device entry off={off}"
                    frame = GuardedBuffers(torch, {"rgb": (ref.shape, np.float32)}, off=off)
                    counter = GuardedBuffers(torch, {"rays": ((2,), np.uint32)}, off=2)  # (a 64-bit counter: 8-byte aligned)
                    torch.cuda.synchronize()
                    gpu.render_device(cam, RV.options(method, shape), frame.ptr("rgb"), counter.ptr("rays"))
                    torch.cuda.synchronize()
                    assert_same_bits(frame.read("rgb"), ref, what, nan_equal=True)  # (read() checks the guard words)
                    lo, hi = (int(x) for x in counter.read("rays"))
                    assert lo | (hi << 32) == ref_rays, what
                    info = gpu.last_launch_info()
                    assert _launch(info) == RV.expected_launch(name, v, method) and info["block_threads"] == 512, (what, info)
                    assert info["lds_bytes"] < gpu.wide_tree()[2] * 512 * 4, (what, info)
    finally:
        _reset(gpu)
