"""CPU reference for the depth-of-field stage (rt_dof, include/rt_hip.h) in numpy float32: every operation of the header's
definition as one f32 array operation, rounded where the header rounds, in the header's order -- the circle of confusion per pixel,
then the gather as a loop over the (2R+1)^2 tap offsets (dy outer, dx inner), vectorised over the frame.  No oracle: the stage uses
nothing but IEEE +, -, *, / and sqrt."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
DEFAULTS = dict(focus_distance=10.0, blur_scale=0.0, max_radius=8, planar_depth=1)
MAX_RADIUS = 16


def workspace_bytes(w, h):
    return -(-8 * w * h // 16) * 16


def _vec(camera, name):
    return np.array(getattr(camera, name)[:], dtype=F32)


def _direction(o, ll, hz, vt, u, v):
    """n(D(u, v)): three components, each an array of the broadcast shape of u and v (or a scalar)"""
    d = [((ll[c] + hz[c] * u) + vt[c] * v) - o[c] for c in range(3)]
    m = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return [d[c] / m for c in range(3)]


def cosines(camera, w, h):
    """cosine(p) of every pixel: (h, w) f32"""
    o, ll, hz, vt = (_vec(camera, k) for k in ("origin", "lower_left", "horizontal", "vertical"))
    u = (np.arange(w, dtype=F32) / F32(w - 1))[None, :]
    v = (F32(1.0) - np.arange(h, dtype=F32) / F32(h - 1))[:, None]
    with np.errstate(all="ignore"):
        n = _direction(o, ll, hz, vt, u, v)
        f = _direction(o, ll, hz, vt, F32(0.5), F32(0.5))
        return ((n[0] * f[0] + n[1] * f[1]) + n[2] * f[2]).astype(F32)


def circle_of_confusion(depth, camera=None, **opts):
    """(r, depthkey, near) of every pixel: (h, w) f32, f32, bool"""
    o = dict(DEFAULTS, **opts)
    t = np.ascontiguousarray(depth, dtype=F32)
    h, w = t.shape
    f = F32(o["focus_distance"])
    with np.errstate(all="ignore"):
        z = (t * cosines(camera, w, h)).astype(F32) if o["planar_depth"] else t
        real = np.isfinite(t) & (t > 0) & (z > 0)
        k = np.where(real, np.minimum(np.abs(z - f) / z, F32(FLT_MAX)), F32(1.0)).astype(F32)
        r = np.maximum(F32(0.5), np.minimum(F32(o["blur_scale"]) * k, F32(o["max_radius"]))).astype(F32)
    key = np.where(real, z, F32(np.inf)).astype(F32)
    return r, key, real & (z < f)


def signed_coc(depth, camera=None, **opts):
    r, _, near = circle_of_confusion(depth, camera, **opts)
    return np.where(near, -r, r).astype(F32)


def gather(img, r, key, R):
    """the gather of the header over an (h, w, 3) frame with the per-pixel radii and depth keys given"""
    img = np.ascontiguousarray(img, dtype=F32)
    h, w, _ = img.shape
    finite = np.isfinite(img).all(axis=2)

    def pad(a, fill):
        return np.pad(a, ((R, R), (R, R)) + ((0, 0),) * (a.ndim - 2), constant_values=fill)

    rp, kp, vp = pad(r, F32(0)), pad(key, F32(np.inf)), pad(finite, False)  # vp: the tap is on the frame and finite
    cp = pad(np.where(finite[..., None], img, F32(0)), F32(0))
    sw = np.full((h, w), -0.0, F32)
    sc = np.full((h, w, 3), -0.0, F32)
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                at = (slice(R + dy, R + dy + h), slice(R + dx, R + dx + w))
                rq, kq = rp[at], kp[at]
                d = np.sqrt(F32(dx * dx + dy * dy))
                re = np.where(kq > key, np.minimum(rq, r), rq)
                cover = np.minimum(np.maximum((re - d) + F32(0.5), F32(0.0)), F32(1.0))
                take = vp[at] & (cover != 0)
                dm = re + re
                wgt = cover / (dm * dm)
                sw = np.where(take, sw + wgt, sw)
                sc = np.where(take[..., None], sc + wgt[..., None] * cp[at], sc)
        out = sc / sw[..., None]
    keep = ~finite | (sw == 0)
    return np.where(keep[..., None], img, out).astype(F32)


def dof(img, depth, camera=None, coc=False, **opts):
    """rt_dof of an (h, w, 3) frame and its (h, w) depth plane; coc=True returns (out, the signed radii)"""
    o = dict(DEFAULTS, **opts)
    r, key, near = circle_of_confusion(depth, camera, **o)
    out = gather(img, r, key, int(o["max_radius"]))
    return (out, np.where(near, -r, r).astype(F32)) if coc else out
