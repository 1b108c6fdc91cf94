"""The cases the GPU tests of rt_render_adaptive run (tests/test_gpu_adaptive_loop.py), and their non-vacuity on the CPU oracle
alone.  A threshold is DERIVED, not guessed: the checker runs min_batches whole-frame batches at a threshold above every error,
the distinct tile errors of that state are sorted, and the threshold is the midpoint of the adjacent pair at position `rank`
(a fraction of the way up the sorted list) -- so the batch after min_batches renders some tiles and not all, by construction."""
import functools

import numpy as np
import pytest

import adaptive_checker as A
import noise_checker as N
import scenes
from tiles_cases import built as _built  # test_gpu_ao.SCENES by name, radiance_cases' scenes by key

abi = scenes.abi
F32 = np.float32
W, H = 24, 20  # 3 x 3 tiles, the bottom row padded
FLOOR = 0.01

# name -> (scene, method, batch, split, min_batches, max_batches, rank, albedo?)
CASES = {
    "materials_mis_high": ("all_materials", abi.RT_METHOD_MIS, 4, 2, 1, 12, 0.8, False),
    "materials_naive_mid": ("all_materials", abi.RT_METHOD_NAIVE, 4, 4, 2, 12, 0.5, True),
    "weekend_mis_low": ("rtweekend1", abi.RT_METHOD_MIS, 2, 2, 1, 4, 0.1, False),
    "shadowed_mis_mid": ("overshadowed", abi.RT_METHOD_MIS, 4, 2, 1, 10, 0.5, False),
    # emissive primitives AND a samplable sky (radiance_cases.SHAPES): the one arm of sample_lights the loop had never run
    "lit_sky_mis_mid": ("shape/primitives_and_sky", abi.RT_METHOD_MIS, 4, 2, 1, 10, 0.5, False),
}


def opts(name):
    scene, method, batch, split, _, _, _, _ = CASES[name]
    o = abi.default_render_opts(W, H, batch, method=method, seed=11)
    o.sample_begin = 3
    o.sample_split = split
    return o


def albedo(name):
    """a fixed synthetic albedo plane (the demodulation is arithmetic on whatever plane it is given)"""
    if not CASES[name][7]:
        return None
    rng = np.random.default_rng(5)
    return (F32(0.05) + F32(0.9) * rng.random((H, W, 3), dtype=np.float32)).astype(F32)


@functools.lru_cache(maxsize=None)
def _passes(name, b):
    scene, _, batch, _, _, _, _, _ = CASES[name]
    _, _, cpu, cam = _built(scene)
    o = opts(name)
    p = N.passes(cpu, cam, o, batch, int(o.sample_begin) + b * batch)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def threshold(name):
    _, _, batch, split, min_batches, _, rank, _ = CASES[name]
    r = A.adaptive(lambda b: _passes(name, b), W, H, batch, split, min_batches, min_batches * batch, FLOOR, np.inf, albedo(name))
    e = np.unique(r["tile_error"][np.isfinite(r["tile_error"])])
    assert len(e) >= 2, f"{name}: all tile errors equal -- replace the scene"
    i = min(int(rank * (len(e) - 1)), len(e) - 2)
    mid = F32((np.float64(e[i]) + np.float64(e[i + 1])) / 2)
    assert e[i] < mid < e[i + 1], (name, e[i], mid, e[i + 1])
    return float(mid)


@functools.lru_cache(maxsize=None)
def checked(name):
    _, _, batch, split, min_batches, max_batches, _, _ = CASES[name]
    return A.adaptive(lambda b: _passes(name, b), W, H, batch, split, min_batches, max_batches * batch, FLOOR, threshold(name), albedo(name))


def test_the_cases_are_not_vacuous():
    n_tiles = 9
    shrinks_twice = ends_converged = ends_at_the_cap = 0
    for name, (_, _, batch, _, min_batches, max_batches, _, _) in CASES.items():
        r = checked(name)
        counts = [len(a) for a in r["active"]]
        assert any(0 < c < n_tiles for c in counts), (name, counts)  # a partial batch by construction
        assert 0 < counts[min_batches - 1] < n_tiles, (name, counts)
        drops = sum(1 for i in range(1, len(counts)) if counts[i] < counts[i - 1])
        shrinks_twice += drops >= 2
        if r["converged"]:
            assert r["batches"] < max_batches or counts[-1] == 0
            assert r["pixel_passes"] < W * H * r["batches"] * batch or r["batches"] == min_batches, (name, r["pixel_passes"])
            ends_converged += r["batches"] < max_batches
            if r["batches"] > min_batches:
                assert r["pixel_passes"] < W * H * r["batches"] * batch
        else:
            assert r["batches"] == max_batches and counts[-1] > 0
            ends_at_the_cap += 1
        # a stopped tile never restarts: the active sets are nested
        for prev, cur in zip(r["active"], r["active"][1:]):
            assert set(cur.tolist()) <= set(prev.tolist()), name
    assert shrinks_twice >= 1 and ends_converged >= 1 and ends_at_the_cap >= 1, (shrinks_twice, ends_converged, ends_at_the_cap)
    for name in CASES:
        r = checked(name)
        if r["converged"]:
            assert r["pixel_passes"] < W * H * r["batches"] * CASES[name][2], name
