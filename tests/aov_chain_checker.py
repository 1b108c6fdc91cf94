"""CPU reference for the specular-chain AOV buffers (rt_render_aov_chain, include/rt_hip.h): the definition restated in numpy
float32 over the oracle's pieces.

  segment 0   the camera ray of tests/aov_checker.py (primary_rays: the first two draws of (seed, pixel, pass)); no other draw
  hits        oracle Scene.check_hit on each segment's (origin, un-normalised direction)
  followed    Refract always, Reflect with fuzz <= fuzz_limit, while b < max_chain:
              T *= colour_value(wo, point) of the material's texture (aov_checker.texture_colours), D += t, b += 1
  next ray    Reflect (and Refract beyond the critical angle): offset_ray(point, normal, error, true), reflected(-wo, normal)
              with NO fuzz term; Refract otherwise: offset_ray(..., false) and perp + para of refract.rs:44-48.
              offset_ray is restated over oracle.utility's next_float / previous_float; test_aov_chain.py pins the restatement
              to oracle.offset_ray
  terminal    albedo = T * aov_checker.albedo_of_hits (Lambertian factor, sky rule), normal, depth term D + t, IDs at the first pass
  folds       as aov_checker.aovs: sums in pass order from +0, divided once; bounces = f32 sum of b / spp
"""
import numpy as np

import aov_checker as K
import oracle as O

abi = K.abi
f32 = np.float32
NO_ID = K.NO_ID


def dot(a, b):
    """Vec3::dot: (x*x + y*y) + z*z in f32"""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def offset_rays(point, normal, error, is_brdf):
    """utility::offset_ray (utility/mod.rs:88-117) for [n] hits"""
    offset = dot(np.abs(normal), error)[:, None] * normal
    if not is_brdf:
        offset = -offset
    o = (point + offset).astype(np.float32)
    return np.where(offset > 0, O.utility(0, o), O.utility(1, o)).astype(np.float32)


def reflected(v, normal):
    """Vec3::reflected: 2 * dot(v, n) * n - v"""
    return (f32(2.0) * dot(v, normal))[:, None] * normal - v


def next_segments(materials, h, wo):
    """(origins, un-normalised directions) that continue the chain behind the followed hits `h` (check_hit records) reached
    in normalised directions `wo`; materials: the rt_material_desc of each hit"""
    n = len(h)
    normal, point, error = h["normal"], h["point"], h["error"]
    is_glass = np.array([m.type == abi.RT_MAT_REFRACT for m in materials], dtype=bool)
    eta = np.array([m.param for m in materials], dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        eta_fraction = np.where(h["out"] != 0, f32(1.0) / eta, eta).astype(np.float32)  # refract.rs:28-31
        cos_theta = np.fmin(dot(-wo, normal), f32(1.0))  # f32::min ignores a NaN operand
        sin_theta = np.sqrt(f32(1.0) - cos_theta * cos_theta)
        mirror = ~is_glass | (eta_fraction * sin_theta > f32(1.0))
        perp = eta_fraction[:, None] * (wo + cos_theta[:, None] * normal)
        para = (f32(-1.0) * np.sqrt(np.abs(f32(1.0) - dot(perp, perp))))[:, None] * normal
        d_refract = perp + para
        d_reflect = reflected(-wo, normal)
    o = np.where(mirror[:, None], offset_rays(point, normal, error, True), offset_rays(point, normal, error, False))
    d = np.where(mirror[:, None], d_reflect, d_refract)
    assert o.dtype == np.float32 and d.dtype == np.float32 and o.shape == (n, 3)
    return o, d


def chain_terms(scene, oracle_scene, origins, directions, max_chain=8, fuzz_limit=0.0):
    """the chains that start with the rays (origins, un-normalised directions): per ray the terminal's check_hit record
    ("terminal"), the last segment's normalised direction ("wo"), T [n,3], D [n], b [n] and the per-pass terms "albedo" [n,3],
    "normal" [n,3], "depth" [n] (D + t; meaningful where "hit"), "hit" [n] bool"""
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3).copy()
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3).copy()
    n = len(o)
    fuzz_limit = f32(fuzz_limit)
    T = np.ones((n, 3), np.float32)
    D = np.zeros(n, np.float32)
    b = np.zeros(n, np.int64)
    terminal = np.zeros(n, dtype=O.HIT_DTYPE)
    wo_t = np.zeros((n, 3), np.float32)
    active = np.arange(n)
    while len(active):
        h = oracle_scene.check_hit(o[active], d[active])
        wo = K.normalised(d[active])
        hit = h["index"] != np.uint64(abi.NO_INDEX)
        mats = [scene.materials[int(m)] for m in h["material"]]
        follows = np.array([m.type == abi.RT_MAT_REFRACT or (m.type == abi.RT_MAT_REFLECT and f32(m.param) <= fuzz_limit) for m in mats],
                           dtype=bool)
        follows &= hit & (b[active] < max_chain)
        ends = active[~follows]
        terminal[ends] = h[~follows]
        wo_t[ends] = wo[~follows]
        idx = active[follows]
        if len(idx):
            hf, wf = h[follows], wo[follows]
            mf = [m for m, f in zip(mats, follows) if f]
            colour = np.zeros((len(idx), 3), np.float32)
            for t in {int(m.texture) for m in mf}:
                sel = np.array([int(m.texture) == t for m in mf], dtype=bool)
                colour[sel] = K.texture_colours(scene, t, wf[sel], hf["point"][sel])
            T[idx] = T[idx] * colour
            D[idx] = D[idx] + hf["t"]
            b[idx] += 1
            o[idx], d[idx] = next_segments(mf, hf, wf)
        active = idx
    hit = terminal["index"] != np.uint64(abi.NO_INDEX)
    return {"terminal": terminal, "wo": wo_t, "T": T, "D": D, "b": b, "hit": hit,
            "albedo": T * K.albedo_of_hits(scene, terminal, wo_t), "normal": np.where(hit[:, None], terminal["normal"], f32(0.0)),
            "depth": D + terminal["t"]}


def aovs(scene, oracle_scene, camera, width, height, spp, seed=1, sample_begin=0, pixels=None, max_chain=8, fuzz_limit=0.0):
    """the seven channels for `pixels` (flat indices y*width + x; default all), as rt_render_aov_chain defines them: albedo /
    normal [n, 3], depth / coverage / bounces [n] f32, primitive / material [n] u32"""
    if pixels is None:
        pixels = np.arange(width * height)
    pixels = np.asarray(pixels, dtype=np.int64)
    order = oracle_scene.primitive_order().astype(np.uint64)
    n = len(pixels)
    albedo = np.zeros((n, 3), np.float32)
    normal = np.zeros((n, 3), np.float32)
    t_sum = np.zeros(n, np.float32)
    b_sum = np.zeros(n, np.float32)
    hits_n = np.zeros(n, np.int64)
    prim = mat = None
    for p in range(spp):
        o, d = K.primary_rays(camera, width, height, seed, pixels, sample_begin + p)
        c = chain_terms(scene, oracle_scene, o, d, max_chain, fuzz_limit)
        hit, h = c["hit"], c["terminal"]
        albedo = albedo + c["albedo"]
        normal = normal + c["normal"]
        t_sum = t_sum + np.where(hit, c["depth"], f32(0.0))
        b_sum = b_sum + c["b"].astype(np.float32)
        hits_n += hit
        if p == 0:
            prim = np.where(hit, order[np.where(hit, h["index"], 0).astype(np.int64)], NO_ID).astype(np.uint32)
            mat = np.where(hit, h["material"], NO_ID).astype(np.uint32)
    k = f32(spp)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = np.where(hits_n > 0, t_sum / hits_n.astype(np.float32), f32(0.0)).astype(np.float32)
    return {"albedo": albedo / k, "normal": normal / k, "depth": depth, "coverage": hits_n.astype(np.float32) / k,
            "primitive": prim, "material": mat, "bounces": b_sum / k}
