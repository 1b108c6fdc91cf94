"""CPU reference for the auxiliary buffers through a lens camera (rt_render_lens_aov, include/rt_hip.h), built from pieces that exist:

  segment 0   lens_checker.rays: the ray rt_render_lens makes for the sample, on the camera stream (seed, 2^63 + pixel, pass); the
              `inside` mask names the black fisheye samples
  chain       aov_chain_checker.chain_terms on those rays (oracle check_hit per segment, aov_checker's texture colours, the
              Reflect / Refract continuations); max_chain = 0 is the first hit
  folds       as aov_checker.aovs / aov_chain_checker.aovs: sums in pass order from +0, divided once by the pass count; a black sample
              is skipped -- no term in any sum, not counted toward depth, coverage or bounces; IDs from pass sample_begin, NO_ID if it
              is black

No arithmetic of a ray, a hit or a continuation is restated here."""
import numpy as np

import aov_chain_checker as KC
import lens_checker as LC

f32 = np.float32
NO_ID = KC.NO_ID
CHANNELS = ("albedo", "normal", "depth", "coverage", "primitive", "material", "bounces")


def aovs(scene, oracle_scene, cam, width, height, spp, seed=1, sample_begin=0, max_chain=0, fuzz_limit=0.0, return_inside=False):
    """the seven channels, flat ([n, 3] / [n]), of an abi.LensCamera; return_inside: also the (spp, n) bool mask of the samples
    that are not black"""
    order = oracle_scene.primitive_order().astype(np.uint64)
    n = width * height
    albedo = np.zeros((n, 3), np.float32)
    normal = np.zeros((n, 3), np.float32)
    t_sum = np.zeros(n, np.float32)
    b_sum = np.zeros(n, np.float32)
    hits_n = np.zeros(n, np.int64)
    prim = np.full(n, NO_ID, np.uint32)
    mat = np.full(n, NO_ID, np.uint32)
    masks = []
    for p in range(spp):
        o, d, inside = LC.rays(cam, width, height, seed, (sample_begin + p) & LC.MASK64)
        masks.append(inside)
        idx = np.flatnonzero(inside)
        if not len(idx):
            continue
        c = KC.chain_terms(scene, oracle_scene, o[idx], d[idx], max_chain, fuzz_limit)
        hit, h = c["hit"], c["terminal"]
        albedo[idx] = albedo[idx] + c["albedo"]
        normal[idx] = normal[idx] + c["normal"]
        t_sum[idx] = t_sum[idx] + np.where(hit, c["depth"], f32(0.0))
        b_sum[idx] = b_sum[idx] + c["b"].astype(np.float32)
        hits_n[idx] += hit
        if p == 0:
            prim[idx] = np.where(hit, order[np.where(hit, h["index"], 0).astype(np.int64)], NO_ID).astype(np.uint32)
            mat[idx] = np.where(hit, h["material"], NO_ID).astype(np.uint32)
    k = f32(spp)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = np.where(hits_n > 0, t_sum / hits_n.astype(np.float32), f32(0.0)).astype(np.float32)
    out = {"albedo": albedo / k, "normal": normal / k, "depth": depth, "coverage": hits_n.astype(np.float32) / k,
           "primitive": prim, "material": mat, "bounces": b_sum / k}
    assert all(out[c].dtype == (np.uint32 if c in ("primitive", "material") else np.float32) for c in CHANNELS)
    return (out, np.stack(masks)) if return_inside else out


def framed(r, width, height):
    """flat per-pixel arrays as frames: (H, W, 3) or (H, W)"""
    return {k: v.reshape((height, width, 3) if v.ndim == 2 else (height, width)) for k, v in r.items()}
