"""CPU reference for the first-hit AOV buffers (rt_render_aov, include/rt_hip.h): numpy plus the oracle.

Every step is an IEEE f32 operation in the order the kernels and the oracle use, so the result is bit-exact:
  rays      the first two draws of the stream (seed, y*width + x, pass) as rand's gen_range(0.0..1.0) (rt_detmath.h
            rt_rng_range_f32, from oracle.rng_u32), then u, v and the direction of SimpleCamera::get_ray in the order of
            oracle/ora_render.c's pixel loop and camera_get_ray
  hits      oracle Scene.check_hit on those rays (BVH slot mapped to the rt_scene_desc index through primitive_order)
  albedo    the material's texture at (wo, hit point): Solid, Lerp, Checkered (sin through oracle.detmath), Image (atan2 / acos
            through oracle.detmath) and Perlin restated from textures/mod.rs as the oracle states them; a Lambertian scales
            the colour by its albedo; a miss takes the sky material's texture at point (0, 0, 0) with no factor.
            emit_twin_colours() gets the direction-only textures straight from the oracle instead, for tests that pin the
            restatement to it
  fold      sums in pass order from +0, divided once (include/rt_hip.h)
"""
import copy
import ctypes as C

import numpy as np

import oracle as O
import scenes

abi = scenes.abi
f32 = np.float32
PI = f32(np.pi)
NO_ID = np.uint32(0xFFFFFFFF)


def jitter(seed, pixels, sample):
    """the two jitter draws of (seed, pixel, sample) for every pixel: [n, 2] f32"""
    bits = np.stack([O.rng_u32(seed, int(p), int(sample), 2) for p in pixels])
    unit = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - f32(1.0)
    return unit * f32(1.0) + f32(0.0)  # gen_range(0.0..1.0): value0_1 * (high - low) + low


def primary_rays(camera, width, height, seed, pixels, sample):
    """(origins [n,3], un-normalised directions [n,3]) of pass `sample` for the given pixel indices"""
    pixels = np.asarray(pixels, dtype=np.int64)
    x = (pixels % width).astype(np.float32)
    y = (pixels // width).astype(np.float32)
    j = jitter(seed, pixels, sample)
    u = (j[:, 0] + x) / f32(width - 1)
    v = f32(1.0) - (j[:, 1] + y) / f32(height - 1)
    o = np.array(camera.origin[:], dtype=np.float32)
    ll = np.array(camera.lower_left[:], dtype=np.float32)
    hz = np.array(camera.horizontal[:], dtype=np.float32)
    vt = np.array(camera.vertical[:], dtype=np.float32)
    d = ((ll[None, :] + hz[None, :] * u[:, None]) + vt[None, :] * v[:, None]) - o[None, :]
    return np.broadcast_to(o, d.shape).copy(), d.astype(np.float32)


def normalised(d):
    """Ray::new's direction.normalise(): d / sqrt(dot(d, d)), dot summed x, y, z"""
    m = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d / m[:, None]


def _f32_as_i32(f):
    out = np.where(np.isnan(f), 0.0, np.clip(f, -2147483648.0, 2147483647.0))
    return out.astype(np.int64)


def _f32_as_index(f):
    f = np.where(np.isnan(f) | ~(f > 0), f32(0.0), f).astype(np.float64)
    return np.minimum(np.floor(f), 2.0 ** 63).astype(np.uint64)


def _perlin(tex, p):
    vecs = np.ctypeslib.as_array(tex.perlin_ran_vecs, shape=(256 * 3,)).reshape(256, 3)
    perm = np.ctypeslib.as_array(tex.perlin_perm, shape=(3 * 256,)).reshape(3, 256)
    fl = np.floor(p)
    u, v, w = (p[:, k] - fl[:, k] for k in range(3))
    i, j, k = (_f32_as_i32(fl[:, a]) for a in range(3))
    uu = u * u * (f32(3.0) - f32(2.0) * u)
    vv = v * v * (f32(3.0) - f32(2.0) * v)
    ww = w * w * (f32(3.0) - f32(2.0) * w)
    value = np.zeros(p.shape[0], dtype=np.float32)
    one = f32(1.0)
    for index in range(8):
        ii, jj, kk = index // 4, (index // 2) % 2, index % 2
        a = perm[0][(i + ii) & 255] ^ perm[1][(j + jj) & 255] ^ perm[2][(k + kk) & 255]
        c = vecs[a & 255]
        fi, fj, fk = f32(ii), f32(jj), f32(kk)
        dot = (c[:, 0] * (u - fi) + c[:, 1] * (v - fj)) + c[:, 2] * (w - fk)
        value = value + (((fi * uu + (one - fi) * (one - uu)) * (fj * vv + (one - fj) * (one - vv))) *
                         (fk * ww + (one - fk) * (one - ww))) * dot
    return f32(0.5) * (one + value)


def texture_colours(scene, tex_index, wo, point):
    """colour_value(wo, point) of texture `tex_index` of SceneDescription `scene` for [n] rays: [n, 3] f32"""
    t = scene.textures[tex_index]
    n = wo.shape[0]
    c1 = np.array(t.colour_one[:], dtype=np.float32)
    c2 = np.array(t.colour_two[:], dtype=np.float32)
    if t.type == abi.RT_TEX_SOLID:
        return np.broadcast_to(c1, (n, 3)).copy()
    if t.type == abi.RT_TEX_LERP:
        tt = wo[:, 2] * f32(0.5) + f32(0.5)
        return c1[None, :] * tt[:, None] + c2[None, :] * (f32(1.0) - tt)[:, None]
    if t.type == abi.RT_TEX_CHECKERED:
        s = O.detmath(0, f32(10.0) * point[:, 0]) * O.detmath(0, f32(10.0) * point[:, 1]) * O.detmath(0, f32(10.0) * point[:, 2])
        return np.where((s > 0)[:, None], c1[None, :], c2[None, :])
    if t.type == abi.RT_TEX_IMAGE:
        w, h = int(t.image_width), int(t.image_height)
        img = np.ctypeslib.as_array(t.image_rgb, shape=(w * h * 3,)).reshape(-1, 3)
        phi = O.detmath(3, wo[:, 1], wo[:, 0]) + PI
        theta = O.detmath(2, wo[:, 2])
        uvx = phi / (f32(2.0) * PI)
        uvy = theta / PI
        xp = _f32_as_index(f32(w - 1) * uvx)
        yp = _f32_as_index(f32(h - 1) * uvy)
        index = np.minimum(yp * np.uint64(w) + xp, np.uint64(w * h - 1))
        return img[index.astype(np.int64)]
    if t.type == abi.RT_TEX_PERLIN:
        return np.repeat(_perlin(t, point)[:, None], 3, axis=1)
    return np.ones((n, 3), dtype=np.float32)


def albedo_of_hits(scene, hits, wo):
    """per-pass albedo of check_hit records `hits` for normalised directions `wo`: [n, 3] f32"""
    out = np.zeros((hits.shape[0], 3), dtype=np.float32)
    hit = hits["index"] != np.uint64(abi.NO_INDEX)
    for m in np.unique(hits["material"]):
        sel = hits["material"] == m
        mat = scene.materials[int(m)]
        c = texture_colours(scene, int(mat.texture), wo[sel], hits["point"][sel])
        if mat.type == abi.RT_MAT_LAMBERTIAN:
            c = np.where(hit[sel][:, None], c * f32(mat.param), c)
        out[sel] = c
    return out


def emit_twin(scene):
    """a copy of `scene` whose every material (the sky's included) is Emit(strength 1.0) over the same texture: one naive
    sample of a ray then returns exactly the colour of that texture in the ray's direction (at an offset point)"""
    twin = copy.copy(scene)
    twin.materials = []
    for m in scene.materials:
        e = abi.MaterialDesc()
        C.memmove(C.byref(e), C.byref(m), C.sizeof(e))
        e.type, e.param = abi.RT_MAT_EMIT, 1.0
        twin.materials.append(e)
    return twin


def emit_twin_colours(twin_oracle, origins, directions):
    """one naive sample per ray on an oracle scene built from emit_twin(): [n, 3] f32"""
    out = np.zeros((len(origins), 3), dtype=np.float32)
    for i in range(len(origins)):
        out[i] = twin_oracle.integrate_ray(origins[i], directions[i], abi.RT_METHOD_NAIVE, 1, seed=1, n_threads=1)
    return out


def aovs(scene, oracle_scene, camera, width, height, spp, seed=1, sample_begin=0, pixels=None):
    """the six channels for `pixels` (flat indices y*width + x; default all), as rt_render_aov defines them:
    albedo / normal [n, 3], depth / coverage [n] f32, primitive / material [n] u32"""
    if pixels is None:
        pixels = np.arange(width * height)
    pixels = np.asarray(pixels, dtype=np.int64)
    order = oracle_scene.primitive_order().astype(np.uint64)
    n = len(pixels)
    albedo = np.zeros((n, 3), np.float32)
    normal = np.zeros((n, 3), np.float32)
    t_sum = np.zeros(n, np.float32)
    hits_n = np.zeros(n, np.int64)
    prim = mat = None
    for p in range(spp):
        o, d = primary_rays(camera, width, height, seed, pixels, sample_begin + p)
        h = oracle_scene.check_hit(o, d)
        hit = h["index"] != np.uint64(abi.NO_INDEX)
        albedo = albedo + albedo_of_hits(scene, h, normalised(d))
        normal = normal + np.where(hit[:, None], h["normal"], f32(0.0))
        t_sum = t_sum + np.where(hit, h["t"], f32(0.0))
        hits_n += hit
        if p == 0:
            prim = np.where(hit, order[np.where(hit, h["index"], 0).astype(np.int64)], NO_ID).astype(np.uint32)
            mat = np.where(hit, h["material"], NO_ID).astype(np.uint32)
    k = f32(spp)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = np.where(hits_n > 0, t_sum / hits_n.astype(np.float32), f32(0.0)).astype(np.float32)
    return {"albedo": albedo / k, "normal": normal / k, "depth": depth,
            "coverage": hits_n.astype(np.float32) / k, "primitive": prim, "material": mat}


def tile_pixels(width, height, tiles):
    """flat pixel indices of the 8 x 8 tiles (tx, ty), clipped to the image"""
    out = []
    for tx, ty in tiles:
        for y in range(ty * 8, min(ty * 8 + 8, height)):
            for x in range(tx * 8, min(tx * 8 + 8, width)):
                out.append(y * width + x)
    return np.array(out, dtype=np.int64)


def emit_scene():
    """every material Emit(1.0) over Solid or Lerp, a Lerp sky (Emit 1.0): one naive pass returns the texture colour"""
    sc = scenes.SceneDescription()
    sc.sphere((0, -1000, 0), 1000.0, sc.emissive(sc.solid((0.3, 0.5, 0.2)), 1.0))
    sc.sphere((-1.0, 0.6, 0), 0.6, sc.emissive(sc.lerp((0.9, 0.2, 0.1), (0.1, 0.3, 0.8)), 1.0))
    sc.sphere((1.0, 0.5, 0.5), 0.5, sc.emissive(sc.solid((0.7, 0.7, 0.2)), 1.0))
    n = (0.0, 0.0, 1.0)
    sc.triangle([(-2, 0, -1), (2, 0, -1), (0, 2.5, -1)], [n, n, n], sc.emissive(sc.lerp((0.2, 0.9, 0.4), (0.6, 0.1, 0.5)), 1.0))
    sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (0, 0))
    return sc


EMIT_CAMERA = dict(origin=(0.0, 1.2, 5.0), lookat=(0.0, 0.6, 0.0), vup=(0.0, 1.0, 0.0), fov=50.0,
                   aspect_ratio=float(np.float32(16.0) / np.float32(9.0)), aperture=0.0, focus_dist=10.0)
