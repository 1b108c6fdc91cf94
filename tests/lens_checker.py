"""The lens cameras of include/rt_hip.h (rt_lens_camera, rt_render_lens) restated in numpy float32, written from the header text.

Every operation is one IEEE f32 operation on arrays (numpy rounds each to f32, as the kernels do with contraction off), sums of three
terms run left to right, sines and cosines are the oracle's rt_sinf / rt_cosf (oracle.detmath), square roots and divisions numpy's
(correctly rounded).  The draws of the camera stream (seed, 2^63 + pixel, pass) come from oracle.rng_f32: rt_rng_f32 is
(u >> 8) * 2^-24 of the stream's next word u, and rt_rng_range_f32(0, 1) of the same word is (u >> 9) * 2^-23 (times 1, plus 0),
so the jitter is recovered from the f32 draw exactly.  Draws 0 and 1 are the jitter, draws 2 and 3 the lens point.

A sample's value is the oracle's fixed-ray integrator on the sample's ray on the stream (seed, pixel, pass) with one sample: no
arithmetic of a path is restated here.  The fold is rt_render_opts' (noise_checker.chunk_bounds gives the chunks).

  basis(params)                          right, up, forward and the two scalars rt_lens_camera_new must write
  rays(cam, w, h, seed, n)               origins [w*h, 3], directions [w*h, 3], inside [w*h] of pass n (an absolute sample index)
  pass_image(cpu, cam, w, h, ...)        (h, w, 3) f32: pass n, black samples +0; the inside mask; on request each sample's ray count
  fold(passes, split)                    the frame and, for split > 1, the chunk sums (S, h, w, 3)
  frame(cpu, cam, opts, split)           both, the number of inside samples and, on request, rays_shot
  tiled(sums, w, h)                      chunk sums in rt_render_lens' layout (S, tiles, 8, 8, 3), padding +0
"""
import numpy as np

import noise_checker as N

F32 = np.float32
PI, TAU, FRAC_PI_2 = F32(3.14159274101257324219), F32(6.28318548202514648438), F32(1.57079637050628662109)
PERSPECTIVE, ORTHOGRAPHIC, FISHEYE, EQUIRECT = range(4)
CAMERA_STREAM = 1 << 63
MASK64 = (1 << 64) - 1


def _v(field):
    return np.array(field[:], dtype=F32)


def basis(origin, lookat, vup, fov, aspect_ratio, aperture, focus_dist):
    """SimpleCamera::new's u, v and -w (camera.rs:32-34), lens_radius (camera.rs:51) and the fisheye's half angle, in f32"""
    def normalised(a):
        return (a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])).astype(F32)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=F32)
    o, l, up = (np.array(x, dtype=F32) for x in (origin, lookat, vup))
    w = normalised(o - l)
    u = normalised(cross(w, up))
    v = cross(u, w)
    return {"right": u, "up": v, "forward": -w, "lens_radius": F32(aperture) / F32(2.0),
            "fisheye_half_angle": (F32(fov) * (PI / F32(180.0))) / F32(2.0)}


def camera_draws(seed, w, h, n):
    """[w*h, 4] f32: the first four rt_rng_f32 draws of every pixel's camera stream at pass n"""
    import oracle as O
    return np.stack([O.rng_f32(seed, CAMERA_STREAM + p, n & MASK64, 4) for p in range(w * h)])


def jitter_from_f32(draw):
    """rt_rng_range_f32(0, 1) of the word whose rt_rng_f32 is `draw`"""
    k = (draw * F32(2.0 ** 24)).astype(np.uint32)  # u >> 8, exact
    return ((k >> 1).astype(F32) * F32(2.0 ** -23)).astype(F32)


def _sin(a):
    import oracle as O
    return O.detmath(0, np.ascontiguousarray(a, dtype=F32))


def _cos(a):
    import oracle as O
    return O.detmath(1, np.ascontiguousarray(a, dtype=F32))


def _sum3(a, b, c):
    return ((a + b) + c).astype(F32)


def rays(cam, w, h, seed, n):
    """the rays of pass n of an abi.LensCamera: (origins [w*h, 3] f32, directions [w*h, 3] f32 as handed to Ray::new, inside [w*h]
    bool -- False: the sample is black and its ray is not to be used)"""
    p = np.arange(w * h)
    x, y = (p % w).astype(F32), (p // w).astype(F32)
    d = camera_draws(seed, w, h, n)
    jx, jy = jitter_from_f32(d[:, 0]) + x, jitter_from_f32(d[:, 1]) + y
    s = (jx / F32(w - 1)).astype(F32)
    t = (F32(1.0) - jy / F32(h - 1)).astype(F32)
    s1, t1 = s[:, None], t[:, None]
    origin, ll, hz, vt = (_v(getattr(cam.pinhole, k))[None, :] for k in ("origin", "lower_left", "horizontal", "vertical"))
    right, up, fwd = (_v(getattr(cam, k))[None, :] for k in ("right", "up", "forward"))
    inside = np.ones(w * h, dtype=bool)
    with np.errstate(all="ignore"):
        if cam.projection == PERSPECTIVE:
            o = np.broadcast_to(origin, (w * h, 3)).copy()
            dirs = (_sum3(ll, hz * s1, vt * t1) - origin).astype(F32)
            lens_radius = F32(cam.lens_radius)
            if lens_radius != 0:
                r = lens_radius * np.sqrt(d[:, 2])
                phi = TAU * d[:, 3]
                off = (right * (r * _cos(phi))[:, None] + up * (r * _sin(phi))[:, None]).astype(F32)
                o, dirs = (o + off).astype(F32), (dirs - off).astype(F32)
        elif cam.projection == ORTHOGRAPHIC:
            o = _sum3(ll, hz * s1, vt * t1)
            dirs = np.broadcast_to(fwd, (w * h, 3)).copy()
        elif cam.projection == FISHEYE:
            a = F32(2.0) * s - F32(1.0)
            b = (F32(2.0) * t - F32(1.0)) * (F32(h - 1) / F32(w - 1))
            rho = np.sqrt(a * a + b * b)
            inside = rho <= F32(1.0)  # False for NaN
            theta = rho * F32(cam.fisheye_half_angle)
            sin_t = _sin(theta)
            dirs = _sum3(right * (sin_t * (a / rho))[:, None], up * (sin_t * (b / rho))[:, None], fwd * _cos(theta)[:, None])
            dirs[rho == 0] = fwd
            o = np.broadcast_to(origin, (w * h, 3)).copy()
        elif cam.projection == EQUIRECT:
            lon = (F32(2.0) * s - F32(1.0)) * PI
            lat = (F32(2.0) * t - F32(1.0)) * FRAC_PI_2
            cos_lat = _cos(lat)
            dirs = _sum3(right * (cos_lat * _sin(lon))[:, None], up * _sin(lat)[:, None], fwd * (cos_lat * _cos(lon))[:, None])
            o = np.broadcast_to(origin, (w * h, 3)).copy()
        else:
            raise ValueError(f"unknown projection {cam.projection}")
    assert o.dtype == F32 and dirs.dtype == F32
    return o, dirs, inside


def pass_image(cpu, cam, w, h, method, seed, n, max_depth=50, rr_threshold=3, return_rays=False):
    """((h, w, 3) f32, (h, w) bool): pass n of the frame -- the integrator's sample on stream (seed, pixel, n) from its first draw
    along the pass's ray; +0 where the sample is outside the fisheye's circle.  return_rays: a third value, (h, w) uint64, the
    integrator's ray count of each sample (the oracle's counted fixed-ray entry); a black sample counts 0"""
    o, d, inside = rays(cam, w, h, seed, n)
    out = np.zeros((w * h, 3), dtype=F32)
    shot = np.zeros(w * h, dtype=np.uint64)
    for p in np.flatnonzero(inside):
        v, shot[p] = cpu.integrate_ray(o[p], d[p], method, n_samples=1, seed=seed, max_depth=max_depth, rr_threshold=rr_threshold, n_threads=1,
                                       stream=int(p), sample_begin=n & MASK64, return_rays=True)
        out[p] = v.astype(F32)  # (the f64 mean of one f32 sample is that sample)
    if return_rays:
        return out.reshape(h, w, 3), inside.reshape(h, w), shot.reshape(h, w)
    return out.reshape(h, w, 3), inside.reshape(h, w)


def fold(passes, split):
    """(frame (h, w, 3), sums (S, h, w, 3) or None): rt_render_opts' fold of (spp, h, w, 3) pass images in pass order"""
    spp = len(passes)
    with np.errstate(all="ignore"):
        if split == 1:
            mean = np.zeros(passes.shape[1:], F32)
            for i in range(spp):
                mean = (mean + (passes[i] - mean) / F32(i + 1)).astype(F32)
            return mean, None
        sums = N.chunk_sums(passes, split, N.chunk_bounds(spp, split))
        return N.combine(sums, spp).astype(F32), sums


def frame(cpu, cam, opts, split, passes=None, return_rays=False):
    """(frame, sums or None, inside samples): rt_render_lens under `opts` at the resolved split; `passes` ((spp, h, w, 3), (spp, h, w))
    reuses pass images computed before.  return_rays: a fourth value, the frame's rays_shot -- the per-sample ray counts summed
    (`passes` then carries them as its third array, (spp, h, w) uint64)"""
    w, h, spp, begin = int(opts.width), int(opts.height), int(opts.samples_per_pixel), int(opts.sample_begin)
    if passes is None:
        got = [pass_image(cpu, cam, w, h, int(opts.render_method), int(opts.seed), (begin + k) & MASK64, int(opts.max_depth),
                          int(opts.rr_threshold), return_rays=True) for k in range(spp)]
        passes = tuple(np.stack([g[i] for g in got]) for i in range(3))
    img, sums = fold(passes[0], split)
    if return_rays:
        return img, sums, int(passes[1].sum()), int(passes[2].sum())
    return img, sums, int(passes[1].sum())


def tiled(sums, w, h):
    """(S, h, w, 3) -> (S, tiles, 8, 8, 3): rt_render_lens' chunk buffer, tiles ascending, padding lanes +0"""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    padded = np.zeros((len(sums), 8 * ty, 8 * tx, 3), F32)
    padded[:, :h, :w] = sums
    return np.ascontiguousarray(padded.reshape(len(sums), ty, 8, tx, 8, 3).transpose(0, 1, 3, 2, 4, 5).reshape(len(sums), ty * tx, 8, 8, 3))


# ---- the state walk of a lane of lens_kernel (csrc/rt_lens.hip), restated: FINISH / CLAIM / START, one loop trip at a time ----
def lane_trips(black, chunk_begin, chunk_end, limit=10000):
    """One lane that claimed a pixel whose chunk is the passes [chunk_begin, chunk_end); black[k]: pass k is outside the circle.
    Returns (trips until the lane claims again, the passes it folded in order, walks it entered).  Each trip is the kernel's loop
    body: FINISH (if the lane waits there: fold, pass += 1, then START or CLAIM), CLAIM (here: the end of the walk), START (if the
    lane waits there: black -> FINISH without a walk, else -> CLOSEST), then the wave's walk, which ends a path (-> FINISH) here
    in one trip and does nothing for a lane in FINISH."""
    ph, k, folded, walks = "START", chunk_begin, [], 0  # (CLAIM set R_PASS = chunk_begin and ph = START)
    for trip in range(1, limit + 1):
        if ph == "FINISH":
            folded.append(k)
            k += 1  # rec[R_PASS] = k: every FINISH advances the counter, black or not
            ph = "CLAIM" if k == chunk_end else "START"
        if ph == "CLAIM":
            return trip, folded, walks
        if ph == "START":
            ph = "FINISH" if black[k] else "CLOSEST"
        # the break test: some lane is not DONE (this one), so the loop goes on; then path_lane_walk
        if ph == "CLOSEST":
            walks += 1
            ph = "FINISH"
    raise AssertionError("the lane never claimed again")
