"""Temporal accumulation with camera reprojection (rt_denoise_temporal, include/rt_hip.h) restated from the header text.

The per-pixel stage -- prepass, reprojection, the four bilinear history taps, the exponential moving averages and the moments'
variance -- is computed in numpy float32 in the header's operation order, so the GPU must match it BIT FOR BIT (motion, n, m1, m2,
n^, z).  It reads the history the GPU wrote for the previous frame (`history_in`), so each step is checked on its own and errors do
not compound over a sequence.  The A-Trous filter that follows is delegated to tests/denoise_checker.py (float64), as in the
denoiser's own tests: e_1 and out are held to a relative tolerance.

A history is a (3, H, W, 4) float32 array: H0 = (e_1.rgb, n), H1 = (n^.xyz, z), H2 = (m1, m2, 0, 0)."""
import numpy as np

import denoise_checker as K

F32 = np.float32
DEFAULTS = dict(alpha_color=0.2, alpha_moments=0.2, depth_tolerance=0.1, normal_tolerance=0.9, max_history=32)


def lum32(e):
    return (F32(0.2126) * e[..., 0] + F32(0.7152) * e[..., 1]) + F32(0.0722) * e[..., 2]


def dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross32(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def camera_vectors(cam):
    """(o, ll, h, vv) float32 (3,) from an abi.Camera, or a (4, 3) array-like in that order"""
    if hasattr(cam, "origin"):
        return tuple(np.array(list(getattr(cam, f)), F32) for f in ("origin", "lower_left", "horizontal", "vertical"))
    a = np.asarray(cam, F32).reshape(4, 3)
    return a[0], a[1], a[2], a[3]


def history_array(raw, h, w):
    """a history buffer's bytes (or float32 data) as (3, H, W, 4) float32"""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), F32).reshape(3, h, w, 4)


def prepass(color, albedo=None, normal=None):
    """(d, e0, l, valid, n^) in float32, as the prepass of rt_denoise without a variance input"""
    c = np.asarray(color, F32)
    h, w = c.shape[:2]
    d = np.fmax(np.asarray(albedo, F32), F32(1e-3)) if albedo is not None else np.ones((h, w, 3), F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e0 = c / d
        l = lum32(e0)
    valid = np.isfinite(c).all(axis=-1) & np.isfinite(l)
    nh = np.zeros((h, w, 3), F32)
    if normal is not None:
        n = np.asarray(normal, F32)
        length = np.sqrt(dot32(n, n))
        with np.errstate(invalid="ignore", divide="ignore"):
            nh = np.where((length != 0)[..., None], n / length[..., None], F32(0)).astype(F32)
    return d, e0, l, valid, nh


def step(color, depth, cam, prev=None, history_in=None, albedo=None, normal=None, **opts):
    """The per-pixel stage of one frame.  Returns a dict of float32 arrays: motion (H, W, 2), e (H, W, 3), n, m1, m2, nh
    (H, W, 3), z, valid (bool), var (float64: the moments' variance where n >= 4, the denoiser checker's 5 x 5 estimate elsewhere),
    d, and `history` (3, H, W, 4) as the GPU writes it before the feedback (H0.rgb = e; the GPU then stores e_1 there)."""
    o_ = dict(DEFAULTS, **{k: v for k, v in opts.items() if k in DEFAULTS})
    a_c, a_m = F32(o_["alpha_color"]), F32(o_["alpha_moments"])
    z_tol, n_tol, max_h = F32(o_["depth_tolerance"]), F32(o_["normal_tolerance"]), F32(o_["max_history"])
    d, e0, l, valid, nh = prepass(color, albedo, normal)
    z = np.asarray(depth, F32)
    h, w = z.shape
    fw, fh = F32(w - 1), F32(h - 1)
    xc = np.arange(w, dtype=F32)[None, :] + F32(0.5)
    yc = np.arange(h, dtype=F32)[:, None] + F32(0.5)
    xc, yc = np.broadcast_to(xc, (h, w)), np.broadcast_to(yc, (h, w))
    motion = np.full((h, w, 2), np.nan, F32)
    e, n, m1, m2 = e0.copy(), np.ones((h, w), F32), l.copy(), (l * l).astype(F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if history_in is not None:
            hist = np.asarray(history_in, F32).reshape(3, h, w, 4)
            o, ll, hh, vv = camera_vectors(cam)
            o2, ll2, h2, v2 = camera_vectors(prev)
            u = (xc / fw)[..., None]
            v = (F32(1) - yc / fh)[..., None]
            D = ((ll + hh * u) + vv * v) - o
            dh = D / np.sqrt(dot32(D, D))[..., None]
            hit = (z > 0) & np.isfinite(z)
            miss = z == 0
            R = np.where(hit[..., None], (o + dh * z[..., None]) - o2, dh).astype(F32)
            L = ll2 - o2
            chv = cross32(h2, v2)
            det = dot32(L, chv)
            s = dot32(R, chv) / det
            al = dot32(L, cross32(R, v2)) / det
            be = dot32(L, cross32(h2, R)) / det
            ok = (hit | miss) & (det != 0) & (s > 0) & np.isfinite(s) & np.isfinite(al) & np.isfinite(be)
            X = (al / s) * fw
            Y = (F32(1) - be / s) * fh
            motion[..., 0] = np.where(ok, X - xc, np.nan)
            motion[..., 1] = np.where(ok, Y - yc, np.nan)
            fx, fy = X - F32(0.5), Y - F32(0.5)
            i0, j0 = np.floor(fx), np.floor(fy)
            ax, ay = fx - i0, fy - j0
            bx, by = F32(1) - ax, F32(1) - ay
            dist = np.sqrt(dot32(R, R))
            ztol = z_tol * dist
            np0 = (nh == 0).all(axis=-1)
            zero = np.zeros((h, w), F32)
            sw, s1, s2, nmax = zero.copy(), zero.copy(), zero.copy(), zero.copy()
            se = np.zeros((h, w, 3), F32)
            taps = ((i0, j0, bx * by), (i0 + F32(1), j0, ax * by), (i0, j0 + F32(1), bx * ay), (i0 + F32(1), j0 + F32(1), ax * ay))
            for ti, tj, wk in taps:
                inside = (ti >= 0) & (ti <= fw) & (tj >= 0) & (tj <= fh) & (wk >= F32(1 / 64))
                qi = np.where(inside, ti, 0).astype(np.int64)
                qj = np.where(inside, tj, 0).astype(np.int64)
                q0, q1, q2 = hist[0, qj, qi], hist[1, qj, qi], hist[2, qj, qi]
                acc = ok & valid & inside & (q0[..., 3] >= 1)
                zq = q1[..., 3]
                acc &= np.where(hit, (zq > 0) & (np.abs(zq - dist) <= ztol), zq == 0)
                if normal is not None:
                    nq0 = (q1[..., :3] == 0).all(axis=-1)
                    acc &= np0 | nq0 | (dot32(nh, q1[..., :3]) >= n_tol)
                sw = np.where(acc, sw + wk, sw)
                se = np.where(acc[..., None], se + wk[..., None] * q0[..., :3], se)
                s1 = np.where(acc, s1 + wk * q2[..., 0], s1)
                s2 = np.where(acc, s2 + wk * q2[..., 1], s2)
                nmax = np.where(acc, np.fmax(nmax, q0[..., 3]), nmax)
            have = sw > 0
            ep, m1p, m2p = se / sw[..., None], s1 / sw, s2 / sw
            nn = np.fmin(nmax + F32(1), max_h)
            ac, am = np.fmax(a_c, F32(1) / nn), np.fmax(a_m, F32(1) / nn)
            e = np.where(have[..., None], ep + ac[..., None] * (e0 - ep), e0).astype(F32)
            m1 = np.where(have, m1p + am * (l - m1p), m1).astype(F32)
            m2 = np.where(have, m2p + am * (l * l - m2p), m2).astype(F32)
            n = np.where(have, nn, n).astype(F32)
        e = np.where(valid[..., None], e, F32(0)).astype(F32)
        n = np.where(valid, n, F32(0)).astype(F32)
        m1 = np.where(valid, m1, F32(0)).astype(F32)
        m2 = np.where(valid, m2, F32(0)).astype(F32)
        spatial = K.spatial_variance(K.lum(np.where(valid[..., None], e0.astype(np.float64), 0.0)), valid)
        var = np.where(n >= 4, np.fmax(F32(0), m2 - m1 * m1).astype(np.float64), spatial)
    history = np.zeros((3, h, w, 4), F32)
    history[0, ..., :3], history[0, ..., 3] = e, n
    history[1, ..., :3], history[1, ..., 3] = nh, z
    history[2, ..., 0], history[2, ..., 1] = m1, m2
    return dict(motion=motion, e=e, n=n, m1=m1, m2=m2, nh=nh, z=z, valid=valid, var=var, d=d, history=history)


def filtered(st, color, normal_given, iterations=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=0.1):
    """(e_1, out) float64 of the A-Trous filter on (e, Var) with this frame's guides (denoise_checker): e_1 demodulated (0 at
    invalid pixels, as the history stores it), out = e_N * d, c at invalid pixels"""
    kw = dict(sigma_luminance=sigma_luminance, sigma_normal=sigma_normal, sigma_depth=sigma_depth, exclude=~st["valid"])
    normal = st["nh"] if normal_given else None
    e64 = st["e"].astype(np.float64)
    e1 = K.denoise(e64, normal=normal, depth=st["z"], variance=st["var"], iterations=1, **kw)
    e1 = np.where(st["valid"][..., None], e1, 0.0)
    en = K.denoise(e64, normal=normal, depth=st["z"], variance=st["var"], iterations=iterations, **kw)
    out = np.where(st["valid"][..., None], en * st["d"], np.asarray(color, np.float64))
    return e1, out
