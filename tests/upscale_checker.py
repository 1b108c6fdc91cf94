"""numpy restatement of AOV-guided upscaling (rt_upscale, include/rt_hip.h), written from the header: every operation in float32, in
the header's order.  powf is rt_powf through the oracle (O.detmath(6, x, y)).  Returns the frame and the stage map; the GPU tests
ask for both bit for bit."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(sigma_normal=32.0, depth_tolerance=0.1)
GUIDES = ("albedo", "normal", "depth")


def lum32(rgb):
    """0.2126f*r + 0.7152f*g + 0.0722f*b, left to right, no fma"""
    with np.errstate(all="ignore"):
        return (F32(0.2126) * rgb[..., 0] + F32(0.7152) * rgb[..., 1]) + F32(0.0722) * rgb[..., 2]


def normalise(n):
    """n / |n| per component, 0 where |n| == 0"""
    n = np.asarray(n, F32)
    with np.errstate(all="ignore"):
        length = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        out = n / length[..., None]
    out[length == 0] = 0
    return out.astype(F32)


def powf(O, x, y):
    x = np.ascontiguousarray(x, F32)
    return O.detmath(6, x, np.full(x.shape, y, F32)).reshape(x.shape)


def source_position(n_dst, n_src):
    """fx of every destination column (or row): (((float)x + 0.5f) / (float)(W - 1)) * (float)(w - 1) - 0.5f"""
    x = np.arange(n_dst, dtype=F32)
    return ((x + F32(0.5)) / F32(n_dst - 1)) * F32(n_src - 1) - F32(0.5)


def tent(d):
    return np.fmax(F32(0), F32(1) - np.abs(d) * F32(0.4))


class _Frames:
    """the per-source-pixel and per-destination-pixel quantities of one call"""

    def __init__(self, O, color, W, H, src, dst, sigma_normal, depth_tolerance):
        self.O = O
        c = np.ascontiguousarray(color, F32)
        self.h, self.w = c.shape[:2]
        self.W, self.H = W, H
        src, dst = src or {}, dst or {}
        for k in GUIDES:
            if (src.get(k) is None) != (dst.get(k) is None):
                raise ValueError(f"{k} given at one size only")
        self.use = {k: src.get(k) is not None for k in GUIDES}
        self.sigma, self.tol = F32(sigma_normal), F32(depth_tolerance)
        with np.errstate(all="ignore"):
            d_s = np.fmax(np.asarray(src["albedo"], F32), F32(1e-3)) if self.use["albedo"] else np.ones_like(c)
            e = c / d_s
            self.valid = np.isfinite(c).all(axis=-1) & np.isfinite(lum32(e))
            self.e = np.where(self.valid[..., None], e, F32(0)).astype(F32)
        self.d_d = np.fmax(np.asarray(dst["albedo"], F32), F32(1e-3)) if self.use["albedo"] else np.ones((H, W, 3), F32)
        if self.use["normal"]:
            self.n_s, self.n_d = normalise(src["normal"]), normalise(dst["normal"])
        if self.use["depth"]:
            self.z_s, self.z_d = np.asarray(src["depth"], F32), np.asarray(dst["depth"], F32)

    def guide(self, py, px, qy, qx):
        """g of the taps (qy, qx) (already clamped, integer) for the destination pixels (py, px)"""
        wn = np.ones(py.shape, F32)
        wz = np.ones(py.shape, F32)
        with np.errstate(all="ignore"):
            if self.use["normal"]:
                a, b = self.n_d[py, px], self.n_s[qy, qx]
                dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
                zero = (a == 0).all(axis=-1) | (b == 0).all(axis=-1)
                wn = np.where(zero, F32(1), powf(self.O, np.fmax(F32(0), dot), self.sigma)).astype(F32)
            if self.use["depth"]:
                zp, zq = self.z_d[py, px], self.z_s[qy, qx]
                t = np.abs(zp - zq) / (self.tol * zp)
                near = np.where(t < F32(1), (F32(1) - t) * (F32(1) - t), F32(0))
                wz = np.where((zp == 0) | (zq == 0), np.where((zp == 0) & (zq == 0), F32(1), F32(0)), near).astype(F32)
            return np.where(self.valid[qy, qx], wn * wz, F32(0)).astype(F32)

    def clamp(self, i, j):
        qx = np.fmin(np.fmax(i, F32(0)), F32(self.w - 1)).astype(np.int64)
        qy = np.fmin(np.fmax(j, F32(0)), F32(self.h - 1)).astype(np.int64)
        return qy, qx


def upscale(O, color, W, H, src=None, dst=None, **opts):
    """(out (H, W, 3) float32, stage (H, W) uint8) of an (h, w, 3) frame; src / dst: {"albedo", "normal", "depth"} at the two sizes"""
    o = dict(DEFAULTS, **opts)
    f = _Frames(O, color, W, H, src, dst, o["sigma_normal"], o["depth_tolerance"])
    fx, fy = np.meshgrid(source_position(W, f.w), source_position(H, f.h))
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    i0, j0 = np.floor(fx), np.floor(fy)
    ax, ay = fx - i0, fy - j0
    bx, by = F32(1) - ax, F32(1) - ay
    e_hat = np.zeros((H, W, 3), F32)
    stage = np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        # ---- stage 1
        taps = [(i0, j0, bx * by), (i0 + F32(1), j0, ax * by), (i0, j0 + F32(1), bx * ay), (i0 + F32(1), j0 + F32(1), ax * ay)]
        sw, se = np.zeros((H, W), F32), np.zeros((H, W, 3), F32)
        best_b = np.zeros((H, W), F32)
        nearest = np.zeros((H, W, 3), F32)
        any_valid = np.zeros((H, W), bool)
        for i, j, b in taps:
            qy, qx = f.clamp(i, j)
            bg = b * f.guide(py, px, qy, qx)
            sw = sw + bg
            se = se + bg[..., None] * f.e[qy, qx]
            take = f.valid[qy, qx] & (~any_valid | (b > best_b))  # stage 3's tap: the first valid one, then strictly larger b
            best_b = np.where(take, b, best_b)
            nearest = np.where(take[..., None], f.e[qy, qx], nearest)
            any_valid |= f.valid[qy, qx]
        s1 = sw >= F32(1.0 / 16)
        e_hat[s1] = (se / sw[..., None])[s1]
        stage[s1] = 1
        # ---- stage 2 on the rest
        ry, rx = np.nonzero(~s1)
        if ry.size:
            rfx, rfy, ri0, rj0 = fx[ry, rx], fy[ry, rx], i0[ry, rx], j0[ry, rx]
            sw2, se2 = np.zeros(ry.shape, F32), np.zeros(ry.shape + (3,), F32)
            for dj in (-1, 0, 1, 2):
                for di in (-1, 0, 1, 2):
                    i, j = ri0 + F32(di), rj0 + F32(dj)
                    qy, qx = f.clamp(i, j)
                    wt = (f.guide(ry, rx, qy, qx) * tent(i - rfx)) * tent(j - rfy)
                    sw2 = sw2 + wt
                    se2 = se2 + wt[..., None] * f.e[qy, qx]
            s2 = sw2 >= F32(1.0 / 1024)
            e_hat[ry[s2], rx[s2]] = (se2 / sw2[..., None])[s2]
            stage[ry[s2], rx[s2]] = 2
            # ---- stage 3 / 0
            y3, x3 = ry[~s2], rx[~s2]
            has = any_valid[y3, x3]
            e_hat[y3, x3] = np.where(has[..., None], nearest[y3, x3], F32(0))
            stage[y3, x3] = np.where(has, 3, 0)
        out = (e_hat * f.d_d).astype(F32)
    return out, stage
