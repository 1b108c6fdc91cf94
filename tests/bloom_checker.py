"""numpy restatement of the bloom stage (rt_bloom, include/rt_hip.h), written from the header: float32 throughout, every sum in
the header's order of operations, no fma.  powf is rt_powf through the oracle (O.detmath(6, x, y)); lum is the display checker's."""
import numpy as np

from display_checker import lum32

F32 = np.float32
FLT_MAX = np.finfo(F32).max
MAX_LEVELS = 12
TAIL_PIXELS = 4096  # csrc/rt_bloom.h kBloomTailPixels: what the fused tail holds in LDS
DEFAULTS = dict(threshold=1.0, knee=0.5, intensity=0.05, scatter=0.7, levels=6, exposure_ev=0.0, clamp_max=65504.0, fuse_tail=1)


def level_sizes(w, h, levels):
    """[(w_i, h_i)] of the n levels: halved (rounding up) until `levels` of them or the first of 1 x 1"""
    out = []
    while len(out) < levels:
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
        if (w, h) == (1, 1):
            break
    return out


def workspace_bytes(w, h, levels):
    return sum((12 * a * b + 15) // 16 * 16 for a, b in level_sizes(w, h, levels))


def tail_from(w, h, levels):
    """the first level of the fused tail (csrc/rt_bloom.h bloom_levels): the smallest t >= 1 whose levels t .. n-1 hold at most
    TAIL_PIXELS pixels together; n when there is none"""
    sizes = level_sizes(w, h, levels)
    t, px = len(sizes), 0
    for i in range(len(sizes) - 1, 0, -1):
        px += sizes[i][0] * sizes[i][1]
        if px > TAIL_PIXELS:
            break
        t = i
    return t


def scale(O, ev):
    """s = powf(2.0f, ev)"""
    return O.detmath(6, np.array([2.0], F32), np.array([ev], F32))[0]


def bright(rgb, s, threshold=1.0, knee=0.5, clamp_max=65504.0, **_):
    """the bright pass of an (..., 3) frame at exposure scale s"""
    v = np.asarray(rgb, F32)
    s, th, kn, cm = F32(s), F32(threshold), F32(knee), F32(clamp_max)
    with np.errstate(all="ignore"):
        a = np.where(np.isfinite(v) & (v > 0), v, F32(0)).astype(F32)
        x = np.fmin(a * s, FLT_MAX).astype(F32)
        y = lum32(x)
        over = y > cm
        x = np.where(over[..., None], x * (cm / y)[..., None], x).astype(F32)
        y = np.where(over, cm, y).astype(F32)
        k = th * kn
        q = np.fmin(np.fmax((y - th) + k, F32(0)), F32(2) * k)
        soft = (q * q) / (F32(4) * k + F32(1e-5))
        wgt = np.fmax(soft, y - th) / np.fmax(y, F32(1e-5))
        b = x * wgt[..., None]
    assert b.dtype == F32
    return b


def _reduce_axis(img, axis):
    n = img.shape[axis]
    m = (n + 1) // 2
    X = np.arange(m)
    t = [np.take(img, np.clip(2 * X - 1 + k, 0, n - 1), axis=axis) for k in range(4)]
    return ((t[0] * F32(0.125) + t[1] * F32(0.375)) + t[2] * F32(0.375)) + t[3] * F32(0.125)


def reduce(img):
    """R: (h, w, 3) -> (ceil(h/2), ceil(w/2), 3), horizontal first"""
    return _reduce_axis(_reduce_axis(np.asarray(img, F32), 1), 0)


def _expand_axis(img, n_fine, axis):
    n = img.shape[axis]
    assert n == (n_fine + 1) // 2
    X = np.arange(n_fine)
    even = (X % 2) == 0
    i0 = np.where(even, X // 2 - 1, (X - 1) // 2)
    i1 = np.where(even, X // 2, (X + 1) // 2)
    w0 = np.where(even, F32(0.25), F32(0.75)).astype(F32)
    w1 = np.where(even, F32(0.75), F32(0.25)).astype(F32)
    shape = [1] * img.ndim
    shape[axis] = n_fine
    a = np.take(img, np.clip(i0, 0, n - 1), axis=axis) * w0.reshape(shape)
    b = np.take(img, np.clip(i1, 0, n - 1), axis=axis) * w1.reshape(shape)
    return a + b


def expand(img, w, h):
    """E: a coarse (ceil(h/2), ceil(w/2), 3) image to (h, w, 3), horizontal first"""
    return _expand_axis(_expand_axis(np.asarray(img, F32), w, 1), h, 0)


def pyramid(b, levels, scatter):
    """U_0 of the bright image b (h, w, 3)"""
    h, w = b.shape[:2]
    B, cur = [], b
    for _ in level_sizes(w, h, levels):
        cur = reduce(cur)
        B.append(cur)
    u = B[-1]
    for i in range(len(B) - 2, -1, -1):
        u = B[i] + F32(scatter) * expand(u, B[i].shape[1], B[i].shape[0])
    assert u.dtype == F32
    return u


def bloom(O, rgb, ev=None, **opts):
    """one call on an (H, W, 3) frame.  ev: the exposure the kernels arrive at (state.ev + exposure_ev, summed in f32 by the
    caller); None = opts' exposure_ev"""
    o = dict(DEFAULTS, **opts)
    c = np.asarray(rgb, F32)
    h, w = c.shape[:2]
    s = scale(O, F32(o["exposure_ev"]) if ev is None else F32(ev))
    u0 = pyramid(bright(c, s, **o), o["levels"], o["scatter"])
    with np.errstate(all="ignore"):
        out = c + (F32(o["intensity"]) * expand(u0, w, h)) / s
    assert out.dtype == F32
    return out
