"""The tile render (rt_render_tiles, csrc/rt_adaptive.hip tiles_kernel) on the inputs of tests/tiles_cases.py: every sky regime
through this kernel's own sample_lights / pdf_from_index and its global-memory sky tables, the four arms of sample_lights, chunks
of unequal length, seeds and first samples as 64-bit values, max_depth and rr_threshold off their defaults, and frames smaller
than a tile.  test_tiles_cases.py (CPU) shows that each entry tests something.  The reference is the CPU ORACLE -- its frame, its
ray count, the chunk sums of its passes -- and rt_render on the same device is a second comparison; every frame starts as a
sentinel that the unlisted pixels must keep; the runs with a chunk buffer go through the device entry on guarded buffers, so a
padding lane that is not written shows.  Everything is bit for bit: there is no tolerance in this file."""
import numpy as np
import pytest

import radiance_cases as RC
import scenes
import sky_cases as SK
import tiles_cases as TC
from gpu_support import assert_same_bits
from test_gpu_adaptive import _device_run

pytestmark = pytest.mark.gpu
abi = scenes.abi
SENTINEL = TC.SENTINEL


def _gpu(hb, scene):
    sc, cam_params, _, _ = TC.built(scene)
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


def _check(gpu, cam, key):
    """every list of the entry, with and without a chunk buffer, under every workgroup cap it names, against the oracle; then
    rt_render under the same options against the tile render"""
    import torch
    e, o = TC.ENTRIES[key], TC.opts(key)
    ref, ref_rays = TC.reference(key)
    nan = TC.has_nan(key)  # (printed per entry by test_tiles_cases.py; NaNs compare equal only there)
    every_tile = sorted(t for tiles in e.lists for t in tiles) == list(range(e.n_tiles()))
    last = None
    for groups in e.groups:
        gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, groups)
        for with_sums in e.sums:
            total = 0
            for tiles in e.lists:
                what = f"{key} list {list(tiles)} chunk buffer {with_sums} groups {groups}"
                if with_sums:
                    _, frame, sums, rays = _device_run(torch, gpu, cam, o, list(tiles), sums=True, split=e.split, off=2)
                    assert_same_bits(sums, TC.padded_sums(key, tiles), what + ": chunk sums", nan_equal=nan)
                else:
                    frame = np.full((e.h, e.w, 3), SENTINEL, np.float32)
                    rays, _ = gpu.render_tiles(cam, o, list(tiles), frame)
                m = TC.mask(tiles, e.w, e.h)
                assert_same_bits(frame[m], ref[m], what + ": listed pixels", nan_equal=nan)
                assert (frame[~m].view(np.uint32) == SENTINEL.view(np.uint32)).all(), what + ": a pixel outside the list was written"
                total += rays
                last = frame, m
            if every_tile:  # the counters of a list and of its complement add up to the oracle's rays_shot
                assert total == ref_rays, (key, with_sums, groups, total, ref_rays)
            else:
                assert 0 <= total <= ref_rays, (key, total, ref_rays)
    gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, 0)
    img, rays = gpu.render(cam, o)  # the promise the adaptive loop rests on: the bytes rt_render writes
    frame, m = last
    assert_same_bits(frame[m], img[m], f"{key}: against rt_render", nan_equal=nan)
    assert rays == ref_rays, (key, rays, ref_rays)


# ---- 1. sky regimes through this kernel's sky tables ----
@pytest.mark.parametrize("scene", sorted({TC.ENTRIES[k].scene for k in TC.SKIES}))
def test_sky_regime(hb, scene):
    _, case, base = scene.split("/")
    gpu, cam = _gpu(hb, scene)
    si = gpu.sky_info()
    assert (si["guide_k"], si["inv_res_ok"]) == (SK.CASES[case].guide_k, SK.CASES[case].inv_res_ok)
    _check(gpu, cam, f"{scene}/mis")
    if base == "floor":  # NAIVE never samples the sky: the oracle's bytes under the same texture with sampler_res (0, 0)
        _check(gpu, cam, f"{scene}/naive")


# ---- 2. the four arms of sample_lights ----
@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_sample_lights_arm(hb, name):
    gpu, cam = _gpu(hb, f"shape/{name}")
    si = gpu.sky_info()
    assert (gpu.counts()[2] > 0, (si["res_x"] | si["res_y"]) != 0) == RC.SHAPES[name][0]
    keys = [k for k in TC.ARMS if k.split("/")[1] == name]
    assert len(keys) == 4
    for key in keys:
        _check(gpu, cam, key)


# ---- 3. chunks of unequal length: the whole-pixel path (j, R_TOTAL) and the chunk buffer, one of them under one workgroup ----
@pytest.mark.parametrize("method", ["naive", "mis"])
def test_uneven_chunks(hb, method):
    gpu, cam = _gpu(hb, TC.MATERIALS)
    keys = [k for k in TC.UNEVENS if k.split("/")[1] == method]
    assert [(TC.ENTRIES[k].spp, TC.ENTRIES[k].split) for k in keys] == list(TC.UNEVEN)
    for key in keys:
        _check(gpu, cam, key)


# ---- 4. seeds and first samples as 64-bit values ----
@pytest.mark.parametrize("seed", RC.SEEDS)
@pytest.mark.parametrize("method", ["naive", "mis"])
def test_64_bit_seeds_and_first_samples(hb, method, seed):
    gpu, cam = _gpu(hb, TC.MATERIALS)
    keys = [k for k in TC.STREAMS if k.split("/")[1] == method and TC.ENTRIES[k].seed == seed]
    assert sorted({TC.ENTRIES[k].begin for k in keys}) == sorted(TC.STREAM_BEGINS) and len(keys) == 8
    for key in keys:
        _check(gpu, cam, key)


# ---- 5. depth and roulette ----
@pytest.mark.parametrize("scene", TC.DEPTH_SCENES)
@pytest.mark.parametrize("method", ["naive", "mis"])
def test_depth_and_roulette(hb, method, scene):
    gpu, cam = _gpu(hb, scene)
    keys = [k for k in TC.DEPTH_KEYS if k.split("/")[1:3] == [scene, method]]
    assert len(keys) == 6
    for key in keys:
        _check(gpu, cam, key)


# ---- 6. ragged frames ----
@pytest.mark.parametrize("shape", sorted(TC.RAGGED))
def test_ragged_frames(hb, shape):
    gpu, cam = _gpu(hb, TC.MATERIALS)
    keys = [k for k in TC.RAGGEDS if (TC.ENTRIES[k].w, TC.ENTRIES[k].h) == shape]
    assert len(keys) == 2 * len(TC.RAGGED[shape])
    for key in keys:
        _check(gpu, cam, key)
