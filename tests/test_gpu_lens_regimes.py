"""The lens render (rt_render_lens, csrc/rt_lens.hip lens_kernel) on the inputs of tests/lens_regime_cases.py: every sky regime
through this kernel's view of the tables, the four arms of sample_lights, chunks of unequal length on both item kinds, seeds and
first samples as 64-bit values on the path's stream and on the camera's, max_depth and rr_threshold off their defaults, frames
smaller than a tile and without padding, and the cameras only this entry has.  test_lens_regime_cases.py (CPU) shows that each
entry tests something.  The reference is the CPU ORACLE through lens_checker -- the frame, the chunk sums, and the ray count of the
oracle's counted fixed-ray integrator, sample by sample; the skies whose tables stay in global memory are also compared with
rt_radiance fed the checker's rays.  The runs with a chunk buffer go through the device entry on guarded buffers off alignment, so
a padding lane that is not written shows.  Everything is bit for bit: there is no tolerance in this file, and a NaN equals a NaN
only for an entry whose reference frame holds one (test_lens_regime_cases.py prints them)."""
import numpy as np
import pytest

import lens_regime_cases as LR
import radiance_cases as RC
import scenes
import sky_cases as SK
from gpu_support import GuardedBuffers, assert_same_bits
from test_gpu_lens import _radiance_fold

pytestmark = pytest.mark.gpu
abi = scenes.abi


def _gpu(hb, scene):
    return hb.HipScene(LR.built(scene)[0], device=0)


def _device_run(torch, gpu, cam, o, e, off):
    """the device entry with a chunk buffer, frame and sums `off` floats past a 16-byte boundary (the counter, a u64, on one)"""
    bufs = GuardedBuffers(torch, {"frame": ((e.h, e.w, 3), np.float32), "sums": ((e.split, e.n_tiles(), 8, 8, 3), np.float32)}, off=off)
    count = GuardedBuffers(torch, {"rays": ((2,), np.uint32)}, off=0)
    gpu.render_lens_device(cam, o, bufs.ptr("frame"), bufs.ptr("sums"), count.ptr("rays"))
    torch.cuda.synchronize()
    r = count.read("rays")  # (read() fails if a guard word around the body was overwritten)
    return bufs.read("frame"), bufs.read("sums"), int(r[0]) | (int(r[1]) << 32)


def _check(gpu, cam, key):
    """under every workgroup cap the entry names: the host entry without a chunk buffer, and for S > 1 the device entry with one,
    against the oracle's frame, chunk sums and ray count"""
    import torch
    e, o, ref = LR.ENTRIES[key], LR.opts(key), LR.reference(key)
    nan = ref.has_nan
    for groups in e.groups:
        gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, groups)
        what = f"{key} groups {groups}"
        frame, rays, sums = gpu.render_lens(cam, o)
        assert sums is None
        assert_same_bits(frame, ref.frame, what + ": no chunk buffer", nan_equal=nan)
        assert rays == ref.rays, (what, rays, ref.rays)
        if e.split > 1:
            d_frame, d_sums, d_rays = _device_run(torch, gpu, cam, o, e, off=3)
            assert_same_bits(d_frame, ref.frame, what + ": chunk buffer", nan_equal=nan)
            assert_same_bits(d_sums, ref.tiled, what + ": chunk sums", nan_equal=nan)
            assert (d_sums[:, LR.padding(e.w, e.h)].view(np.uint32) == 0).all(), what + ": a padding lane is not +0"
            assert d_frame.tobytes() == frame.tobytes(), what + ": the chunk buffer changed the frame"
            assert d_rays == ref.rays, (what, d_rays, ref.rays)
    gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, 0)


# ---- 1. sky regimes through this kernel's view of the tables ----
@pytest.mark.parametrize("scene", sorted({LR.ENTRIES[k].scene for k in LR.SKIES}))
def test_sky_regime(hb, scene):
    _, case, base = scene.split("/")
    gpu = _gpu(hb, scene)
    si = gpu.sky_info()
    assert (si["guide_k"], si["inv_res_ok"]) == (SK.CASES[case].guide_k, SK.CASES[case].inv_res_ok)
    keys = [k for k in LR.SKIES if LR.ENTRIES[k].scene == scene]
    assert len(keys) == (4 if base == "floor" else 1)
    for key in keys:  # (NAIVE never samples the sky: the oracle's bytes under the same texture with sampler_res (0, 0))
        _check(gpu, LR.camera(key), key)
    if case in SK.BIG + SK.HUGE:  # the tables stay in global memory: rt_radiance fed the checker's rays, a witness on the GPU
        for key in keys:
            e, ref = LR.ENTRIES[key], LR.reference(key)
            frame, inside = _radiance_fold(gpu, LR.camera(key), e.w, e.h, e.method, e.spp, e.split, e.seed, e.begin)
            assert_same_bits(frame, ref.frame, key + ": rt_radiance on the checker's rays", nan_equal=ref.has_nan)
            assert inside == ref.inside


# ---- 2. the four arms of sample_lights ----
@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_sample_lights_arm(hb, name):
    gpu = _gpu(hb, f"shape/{name}")
    si = gpu.sky_info()
    assert (gpu.counts()[2] > 0, (si["res_x"] | si["res_y"]) != 0) == RC.SHAPES[name][0]
    keys = [k for k in LR.ARMS if k.split("/")[1] == name]
    assert len(keys) == 4
    for key in keys:
        _check(gpu, LR.camera(key), key)


# ---- 3. chunks of unequal length: the whole-pixel path (j, R_TOTAL) and the chunk buffer, (7, 3) also under one workgroup ----
@pytest.mark.parametrize("method", ["naive", "mis"])
def test_uneven_chunks(hb, method):
    gpu = _gpu(hb, LR.MATERIALS)
    keys = [k for k in LR.UNEVENS if k.split("/")[1] == method]
    assert [(LR.ENTRIES[k].spp, LR.ENTRIES[k].split) for k in keys] == list(LR.UNEVEN)
    for key in keys:
        _check(gpu, LR.camera(key), key)


# ---- 4. seeds and first samples as 64-bit values ----
@pytest.mark.parametrize("seed", RC.SEEDS)
@pytest.mark.parametrize("method", ["naive", "mis"])
def test_64_bit_seeds_and_first_samples(hb, method, seed):
    gpu = _gpu(hb, LR.MATERIALS)
    keys = [k for k in LR.STREAMS if k.split("/")[1] == method and LR.ENTRIES[k].seed == seed]
    assert sorted({LR.ENTRIES[k].begin for k in keys}) == sorted(LR.STREAM_BEGINS) and len(keys) == 8
    for key in keys:
        _check(gpu, LR.camera(key), key)


# ---- 5. depth and roulette ----
@pytest.mark.parametrize("scene", LR.DEPTH_SCENES)
@pytest.mark.parametrize("method", ["naive", "mis"])
def test_depth_and_roulette(hb, method, scene):
    gpu = _gpu(hb, scene)
    keys = [k for k in LR.DEPTH_KEYS if k.split("/")[1:3] == [scene, method]]
    assert len(keys) == 6
    for key in keys:
        _check(gpu, LR.camera(key), key)


# ---- 6. ragged frames ----
@pytest.mark.parametrize("shape", sorted(LR.RAGGED))
def test_ragged_frames(hb, shape):
    gpu = _gpu(hb, LR.MATERIALS)
    keys = [k for k in LR.RAGGEDS if (LR.ENTRIES[k].w, LR.ENTRIES[k].h) == shape]
    assert len(keys) == 2 * len(LR.RAGGED[shape])
    for key in keys:
        _check(gpu, LR.camera(key), key)


# ---- 7. what only this entry has ----
@pytest.mark.parametrize("name", sorted({k.split("/")[1] for k in LR.CAMERAS}))
def test_cameras(hb, name):
    gpu = _gpu(hb, LR.MATERIALS)
    keys = [k for k in LR.CAMERAS if k.split("/")[1] == name]
    assert len(keys) == 2
    for key in keys:
        _check(gpu, LR.camera(key), key)
