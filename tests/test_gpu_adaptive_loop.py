"""rt_render_adaptive on the GPU against tests/adaptive_checker.py, bit for bit, on the cases of tests/test_adaptive_cases.py (whose
thresholds are derived on the oracle so that batches are partial), and against rt_render_converged where no tile is ever dropped."""
import numpy as np
import pytest

import scenes
import test_adaptive_cases as T
from gpu_support import assert_same_bits
from tiles_cases import built as _built

pytestmark = pytest.mark.gpu
abi = scenes.abi
W, H = T.W, T.H


def _gpu(hb, scene):
    sc, cam_params, _, _ = _built(scene)
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


def _run(gpu, cam, name, **kw):
    _, _, batch, _, min_batches, max_batches, _, _ = T.CASES[name]
    args = dict(min_batches=min_batches, max_passes=max_batches * batch, albedo=T.albedo(name), luminance_floor=T.FLOOR, threshold=T.threshold(name))
    args.update(kw)
    return gpu.render_adaptive(cam, T.opts(name), batch, **args)


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_against_the_checker(hb, name):
    gpu, cam = _gpu(hb, T.CASES[name][0])
    ref = T.checked(name)
    got = _run(gpu, cam, name)
    for k in ("mean", "variance", "tile_error"):
        assert_same_bits(got[k], ref[k], f"{name} {k}", nan_equal=False)
    assert np.array_equal(got["passes"], ref["passes"]) and got["passes"].dtype == np.uint32
    assert (got["batches"], got["converged"], got["pixel_passes"]) == (ref["batches"], ref["converged"], ref["pixel_passes"])
    assert got["summary"] == ref["summary"], (got["summary"], ref["summary"])
    again = _run(gpu, cam, name)  # no state leaks from one call into the next
    for k in ("mean", "variance", "tile_error", "passes"):
        assert again[k].tobytes() == got[k].tobytes(), k
    assert again["rays_shot"] == got["rays_shot"] and again["batches"] == got["batches"]


@pytest.mark.parametrize("name", ["materials_mis_high", "materials_naive_mid"])
def test_rays_shot_is_the_sum_of_the_batches_rendered_by_hand(hb, name):
    """whole-frame batches through rt_render, masked ones through rt_render_tiles on the checker's own lists"""
    gpu, cam = _gpu(hb, T.CASES[name][0])
    ref = T.checked(name)
    got = _run(gpu, cam, name)
    batch = T.CASES[name][2]
    total = 0
    for b, tiles in enumerate(ref["rendered"]):
        o = T.opts(name)
        o.sample_begin = int(o.sample_begin) + b * batch
        if tiles is None or len(tiles) == 9:
            total += gpu.render(cam, o)[1]
        else:
            total += gpu.render_tiles(cam, o, tiles, np.zeros((H, W, 3), np.float32))[0]
    assert got["rays_shot"] == total


@pytest.mark.parametrize("with_albedo", [False, True])
def test_runs_that_never_drop_a_tile_are_render_converged(hb, with_albedo):
    """threshold 0 runs to max_passes, a threshold above every error stops at min_batches: mean, variance and tile_error are
    rt_render_converged's bytes (which takes no albedo: with one, the mean still is, and the run is held to the checker)"""
    name = "materials_naive_mid"
    gpu, cam = _gpu(hb, T.CASES[name][0])
    batch = T.CASES[name][2]
    for threshold, min_batches, max_batches in ((0.0, 1, 3), (1e30, 2, 5)):
        alb = T.albedo(name) if with_albedo else None
        got = gpu.render_adaptive(cam, T.opts(name), batch, min_batches=min_batches, max_passes=max_batches * batch, albedo=alb,
                                  luminance_floor=T.FLOOR, threshold=threshold)
        conv = gpu.render_converged(cam, T.opts(name), batch, min_batches=min_batches, max_passes=max_batches * batch,
                                    luminance_floor=T.FLOOR, threshold=threshold)
        assert got["batches"] == conv["batches"] == (max_batches if threshold == 0.0 else min_batches)
        assert got["converged"] == conv["converged"] and got["rays_shot"] == conv["rays_shot"]
        assert (got["passes"] == got["batches"] * batch).all() and got["pixel_passes"] == W * H * got["batches"] * batch
        assert got["mean"].tobytes() == conv["mean"].tobytes()
        if not with_albedo:
            assert got["variance"].tobytes() == conv["variance"].tobytes() and got["tile_error"].tobytes() == conv["tile_error"].tobytes()
            assert got["summary"] == conv["summary"]
        else:
            import adaptive_checker as A
            ref = A.adaptive(lambda b: T._passes(name, b), W, H, batch, T.CASES[name][3], min_batches, max_batches * batch, T.FLOOR, threshold, alb)
            for k in ("mean", "variance", "tile_error"):
                assert_same_bits(got[k], ref[k], k, nan_equal=False)
