"""CPU reference for the anti-aliased ID mattes (rt_render_matte, rt_matte_extract, include/rt_hip.h): pure numpy, pure counting.

  pass IDs   pass p's ID of a pixel is, by definition, what rt_render_aov returns in its `primitive` / `material` channel for the
             window [sample_begin + p, sample_begin + p + 1): pass_ids() asks the first-hit checker (tests/aov_checker.py) for exactly
             that, once per pass; a GPU test may hand in the library's own single-pass channels instead
  layers     layers_from_pass_ids(): the 8-slot table filled in pass order, the ranking (count descending, ID ascending), one f32
             division per value
  matte      extract(): the f32 sum of the selected layers' coverages in layer order, clamped to 1
"""
import numpy as np

import aov_checker as K

f32 = np.float32
NO_ID = np.uint32(0xFFFFFFFF)
SLOTS = 8


def layers_from_pass_ids(pass_ids, layers, slots=SLOTS):
    """pass_ids [spp, n] u32 -> (ids [K, n] u32, coverage [K, n] f32, residual [n] f32)"""
    pass_ids = np.asarray(pass_ids, dtype=np.uint32)
    spp, n = pass_ids.shape
    assert 1 <= layers <= slots
    ids = np.full((layers, n), NO_ID, dtype=np.uint32)
    counts = np.zeros((layers, n), dtype=np.int64)
    for q in range(n):
        table = {}  # id -> count, at most `slots` entries; an ID that finds the table full is overflow, whenever it comes
        for v in pass_ids[:, q].tolist():
            if v in table:
                table[v] += 1
            elif len(table) < slots:
                table[v] = 1
        ranked = sorted(table.items(), key=lambda e: (-e[1], e[0]))[:layers]
        for l, (v, c) in enumerate(ranked):
            ids[l, q], counts[l, q] = v, c
    coverage = counts.astype(np.float32) / f32(spp)
    residual = (spp - counts.sum(axis=0)).astype(np.float32) / f32(spp)
    return ids, coverage, residual


def extract(ids, coverage, selection):
    """the matte of `selection` (any order, duplicates allowed) from layers [K, ...]: f32 of the layers' trailing shape"""
    ids, coverage = np.asarray(ids, dtype=np.uint32), np.asarray(coverage, dtype=np.float32)
    chosen = np.isin(ids, np.asarray(selection, dtype=np.uint32).reshape(-1))
    m = np.zeros(ids.shape[1:], dtype=np.float32)
    for l in range(ids.shape[0]):
        m = np.where(chosen[l] & (coverage[l] > 0), m + coverage[l], m).astype(np.float32)
    return np.minimum(m, f32(1.0))


def pass_ids(scene, oracle_scene, camera, w, h, spp, seed, sample_begin, kind, pixels=None):
    """[spp, n] u32: the `kind` ("primitive" / "material") channel of aov_checker.aovs for each single pass of the window"""
    return np.stack([K.aovs(scene, oracle_scene, camera, w, h, 1, seed=seed, sample_begin=sample_begin + p, pixels=pixels)[kind]
                     for p in range(spp)])
