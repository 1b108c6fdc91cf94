"""The A-Trous denoiser of include/rt_hip.h (rt_denoise_opts) restated in numpy float64, written from the header text: (H, W, ...)
arrays in, vectorised over the frame with shifted views.  The GPU computes in f32; tests hold it to this restatement within a
relative tolerance (tests/test_gpu_denoise.py)."""
import numpy as np

F32 = np.float32
LUM = (float(F32(0.2126)), float(F32(0.7152)), float(F32(0.0722)))  # the f32 constants of lum()
ALBEDO_FLOOR = float(F32(1e-3))
EPS = float(F32(1e-6))
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
G3 = (1 / 4, 1 / 2, 1 / 4)


def lum(e):
    return LUM[0] * e[..., 0] + LUM[1] * e[..., 1] + LUM[2] * e[..., 2]


def shifted(a, dy, dx):
    """(b, inside): b[y, x] = a[y + dy, x + dx] where that pixel is in frame (inside True), 0 elsewhere"""
    h, w = a.shape[:2]
    b = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return b, inside


def spatial_variance(l, valid):
    """Var0 without a given variance: over the in-frame valid q of the 5 x 5 box, two passes"""
    s = np.zeros(l.shape)
    count = np.zeros(l.shape)
    taps = []
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            lq, inside = shifted(l, dy, dx)
            vq, _ = shifted(valid, dy, dx)
            m = inside & vq
            taps.append((lq, m))
            s += np.where(m, lq, 0.0)
            count += m
    count = np.maximum(count, 1)  # (invalid p only: their Var is never read)
    mean = s / count
    sq = np.zeros(l.shape)
    for lq, m in taps:
        sq += np.where(m, (lq - mean) ** 2, 0.0)
    return sq / count


def prepare(color, albedo=None, normal=None, depth=None, variance=None, exclude=None):
    """(d, e0, Var0, valid, n^, z) of the prepass; `exclude` marks extra pixels invalid (a test's stand-in for a NaN)"""
    c = np.asarray(color, np.float64)
    h, w = c.shape[:2]
    d = np.fmax(np.asarray(albedo, np.float64), ALBEDO_FLOOR) if albedo is not None else np.ones((h, w, 3))
    valid = np.isfinite(c).all(axis=-1)
    if variance is not None:
        v = np.asarray(variance, np.float64)
        valid &= np.isfinite(v)
    if exclude is not None:
        valid &= ~np.asarray(exclude, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(valid[..., None], c / d, 0.0)
    if variance is not None:
        var = np.where(valid, v, 0.0)
    else:
        var = spatial_variance(lum(e), valid)
    if normal is not None:
        n = np.asarray(normal, np.float64)
        length = np.sqrt((n * n).sum(axis=-1))
        with np.errstate(invalid="ignore", divide="ignore"):
            nh = np.where(length[..., None] > 0, n / np.where(length > 0, length, 1.0)[..., None], 0.0)
    else:
        nh = None
    z = np.asarray(depth, np.float64) if depth is not None else None
    return d, e, var, valid, nh, z


def denoise(color, albedo=None, normal=None, depth=None, variance=None, iterations=5, sigma_luminance=4.0, sigma_normal=128.0,
            sigma_depth=0.1, exclude=None):
    """out (H, W, 3) float64 of the filter in include/rt_hip.h"""
    sigma_luminance, sigma_normal, sigma_depth = (float(F32(x)) for x in (sigma_luminance, sigma_normal, sigma_depth))
    d, e, var, valid, nh, z = prepare(color, albedo, normal, depth, variance, exclude)
    n_zero = (nh == 0).all(axis=-1) if nh is not None else None
    for i in range(iterations):
        k = 2 ** i
        gs = np.zeros(var.shape)
        gw = np.zeros(var.shape)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, inside = shifted(var, dy, dx)
                ok = inside & shifted(valid, dy, dx)[0]
                wg = G3[dx + 1] * G3[dy + 1]
                gs += np.where(ok, wg * vq, 0.0)
                gw += np.where(ok, wg, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            denom = sigma_luminance * np.sqrt(gs / gw) + EPS
        lp = lum(e)
        se = np.zeros(e.shape)
        sw = np.zeros(var.shape)
        sv = np.zeros(var.shape)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                eq, inside = shifted(e, k * dy, k * dx)
                ok = inside & shifted(valid, k * dy, k * dx)[0]
                vq = shifted(var, k * dy, k * dx)[0]
                if dy == 0 and dx == 0:
                    w = np.full(var.shape, 9 / 64)
                else:
                    w = H5[dx + 2] * H5[dy + 2] * np.exp(-np.abs(lp - lum(eq)) / denom)
                    if nh is not None:
                        nq = shifted(nh, k * dy, k * dx)[0]
                        both_zero = n_zero & shifted(n_zero, k * dy, k * dx)[0]
                        wn = np.maximum(0.0, (nh * nq).sum(axis=-1)) ** sigma_normal
                        w = w * np.where(both_zero, 1.0, wn)
                    if z is not None:
                        zq = shifted(z, k * dy, k * dx)[0]
                        with np.errstate(invalid="ignore", divide="ignore"):
                            wz = np.exp(-np.abs(z - zq) / (sigma_depth * z * k))
                        wz = np.where((z == 0) & (zq == 0), 1.0, np.where((z == 0) | (zq == 0), 0.0, wz))
                        w = w * wz
                w = np.where(ok, w, 0.0)
                se += w[..., None] * eq
                sw += w
                sv += w * w * vq
        sw_safe = np.where(valid, sw, 1.0)
        e = np.where(valid[..., None], se / sw_safe[..., None], 0.0)
        var = np.where(valid, sv / (sw_safe * sw_safe), 0.0)
    return np.where(valid[..., None], e * d, np.asarray(color, np.float64))


def halves_variance(a, b, albedo=None):
    """rt_render_denoised's variance, in f32 as the library computes it: (lA - lB) * (lA - lB) * 0.25f, lA = lum(A / d)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    d = np.fmax(np.asarray(albedo, F32), F32(1e-3)) if albedo is not None else np.ones_like(a)

    def lum32(e):
        return (F32(0.2126) * e[..., 0] + F32(0.7152) * e[..., 1]) + F32(0.0722) * e[..., 2]

    la, lb = lum32(a / d), lum32(b / d)
    return ((la - lb) * (la - lb) * F32(0.25)).astype(F32)


def relative_error(got, ref):
    """max |got - ref| / (|ref| + 1e-3 mean |ref|): the tolerance measure of the GPU tests"""
    ref = np.asarray(ref, np.float64)
    scale = np.abs(ref) + 1e-3 * np.abs(ref).mean()
    return float((np.abs(np.asarray(got, np.float64) - ref) / scale).max())
