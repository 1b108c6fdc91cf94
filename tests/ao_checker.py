"""CPU reference for the ambient-occlusion pass (rt_render_ao, include/rt_hip.h): the definition restated in numpy float32 over the
oracle's pieces.

For pixel q and passes s = 0 .. spp-1 of the window [sample_begin, sample_begin + spp):
  camera ray  aov_checker.primary_rays: the first two draws of the stream (seed, q, sample_begin + s) jitter the pixel; a pass whose
              camera ray misses draws nothing more and contributes nothing
  hit         oracle Scene.check_hit; its normal, point and error as they stand
  AO rays     k = 0 .. K-1 in order, on the SAME stream behind the jitter: draws 2 + 2k and 3 + 2k of the stream as rt_rng_f32
              (oracle.rng_f32: every draw, jitter or not, takes one 32-bit word -- test_ao.py pins that) go into
              lambertian_sample (lambertian.rs:5-18) about the hit normal, restated with np.sqrt, oracle.detmath sin / cos and the
              frame coord_from_z in the operation order of csrc/rt_shade.h (pinned against oracle.coord_apply); the origin is
              aov_chain_checker.offset_rays(point, normal, error, is_brdf=True)
  occlusion   check_hit on (origin, d_k): found and not t >= radius; radius 0 = no limit
  folds       integer counts and f32 sums from +0 in (pass, k) order, each value written divided once; with n = hits * K and u the
              rays not occluded:  visibility = n == 0 ? 1 : (float)u / (float)n,
              bent_normal = n == 0 ? 0 : (sum over the rays not occluded of d_k) / (float)n  -- d_k as sampled, not re-normalised
"""
import numpy as np

import aov_checker as K
import aov_chain_checker as C
import oracle as O

abi = K.abi
f32 = np.float32
PI = f32(np.pi)
MAX_RAYS = 64


def ao_draws(seed, pixels, sample, rays_per_pass):
    """[n, 2K] f32: the draws 2 .. 2 + 2K - 1 of the stream (seed, pixel, sample) as rt_rng_f32 makes them"""
    return np.stack([O.rng_f32(seed, int(p), int(sample), 2 + 2 * rays_per_pass)[2:] for p in pixels]).astype(np.float32)


def cross(a, b):
    """Vec3::cross (vec.rs:170-177)"""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(np.float32)


def coord_from_z(z):
    """Coordinate::new_from_z (utility/coord.rs:9-31) for [n] normals: the axes (x, y, z), each [n, 3]"""
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1, 3)
    zero = np.zeros(len(z), np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sx = np.sqrt(z[:, 0] * z[:, 0] + z[:, 2] * z[:, 2])
        sy = np.sqrt(z[:, 1] * z[:, 1] + z[:, 2] * z[:, 2])
        along_x = np.stack([-z[:, 2], zero, z[:, 0]], axis=1) / sx[:, None]
        along_y = np.stack([zero, z[:, 2], -z[:, 1]], axis=1) / sy[:, None]
        x = np.where((np.abs(z[:, 0]) > np.abs(z[:, 1]))[:, None], along_x, along_y).astype(np.float32)
        y = cross(x, z)
    return x, y, z


def to_coord(axes, v):
    """Coordinate::to_coord: v.x * x + v.y * y + v.z * z, summed in that order"""
    x, y, z = axes
    with np.errstate(invalid="ignore", over="ignore"):
        return ((v[:, 0:1] * x + v[:, 1:2] * y) + v[:, 2:3] * z).astype(np.float32)


def lambertian_sample(normal, r1, r2):
    """lambertian.rs:5-18 for [n] normals and the two rt_rng_f32 draws of each: [n, 3] f32, cosine-weighted about the normal"""
    r1, r2 = np.asarray(r1, dtype=np.float32), np.asarray(r2, dtype=np.float32)
    cos_theta = np.sqrt(f32(1.0) - r1)
    sin_theta = np.sqrt(f32(1.0) - cos_theta * cos_theta)
    phi = f32(2.0) * PI * r2
    local = np.stack([O.detmath(1, phi) * sin_theta, O.detmath(0, phi) * sin_theta, cos_theta], axis=1).astype(np.float32)
    return to_coord(coord_from_z(normal), local)


def occluded(oracle_scene, origins, directions, radius):
    """the rule of trace_any with nothing skipped, through check_hit: found and not t >= radius (radius 0: found)"""
    h = oracle_scene.check_hit(origins, directions)
    found = h["index"] != np.uint64(abi.NO_INDEX)
    if radius == 0:
        return found
    return found & ~(h["t"] >= f32(radius))


def ao(oracle_scene, camera, width, height, spp, rays_per_pass=4, radius=0.0, seed=1, sample_begin=0, pixels=None):
    """the two channels for `pixels` (flat indices y*width + x; default all) as rt_render_ao defines them -- "visibility" [n] and
    "bent_normal" [n, 3] f32 -- and the counts behind them: "hits" (passes whose camera ray hit), "rays" (= hits * K) and
    "unoccluded", [n] int64, and "open" [n, spp, K] bool: ray k of pass s was shot and reached nothing"""
    assert 1 <= rays_per_pass <= MAX_RAYS and radius >= 0
    if pixels is None:
        pixels = np.arange(width * height)
    pixels = np.asarray(pixels, dtype=np.int64)
    n_px = len(pixels)
    hits = np.zeros(n_px, np.int64)
    unoccluded = np.zeros(n_px, np.int64)
    bent = np.zeros((n_px, 3), np.float32)
    open_rays = np.zeros((n_px, spp, rays_per_pass), dtype=bool)
    for s in range(spp):
        o, d = K.primary_rays(camera, width, height, seed, pixels, sample_begin + s)
        h = oracle_scene.check_hit(o, d)
        idx = np.nonzero(h["index"] != np.uint64(abi.NO_INDEX))[0]
        if len(idx) == 0:
            continue
        hits[idx] += 1
        h = h[idx]
        origin = C.offset_rays(h["point"], h["normal"], h["error"], True)
        draws = ao_draws(seed, pixels[idx], sample_begin + s, rays_per_pass)
        for k in range(rays_per_pass):
            d_k = lambertian_sample(h["normal"], draws[:, 2 * k], draws[:, 2 * k + 1])
            open_ = ~occluded(oracle_scene, origin, d_k, radius)
            unoccluded[idx] += open_
            open_rays[idx, s, k] = open_
            with np.errstate(invalid="ignore", over="ignore"):
                bent[idx] = np.where(open_[:, None], bent[idx] + d_k, bent[idx])
    rays = hits * rays_per_pass
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nf = rays.astype(np.float32)
        visibility = np.where(rays > 0, unoccluded.astype(np.float32) / nf, f32(1.0)).astype(np.float32)
        bent_normal = np.where((rays > 0)[:, None], bent / nf[:, None], f32(0.0)).astype(np.float32)
    return {"visibility": visibility, "bent_normal": bent_normal, "hits": hits, "rays": rays, "unoccluded": unoccluded,
            "open": open_rays}
