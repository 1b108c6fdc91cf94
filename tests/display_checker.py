"""numpy restatement of the display stage (rt_display, include/rt_hip.h), written from the header: float32 for the per-pixel
arithmetic, float64 for the metering, in the header's order of operations.  powf is rt_powf through the oracle
(O.detmath(6, x, y)); Philox4x32-10 is a vectorised numpy port that tests/test_display.py pins to the oracle's."""
import math

import numpy as np

F32 = np.float32
BINS = 256
# log2(1 + (m + 0.5) / 8), the header's f32 literals
L = [F32(s) for s in ("0.0874628413", "0.247927513", "0.392317423", "0.523561956",
                      "0.643856190", "0.754887502", "0.857980995", "0.954196310")]
FIXED, AUTO = 0, 1
CLAMP, REINHARD, ACES, HABLE = 0, 1, 2, 3
SRGB, GAMMA, LINEAR = 0, 1, 2
ROUND, DITHER, REFERENCE = 0, 1, 2
RGBA8, BGRA8, RGB8 = 0, 1, 2

DEFAULTS = dict(exposure_mode=AUTO, tonemap=ACES, transfer=SRGB, quantiser=DITHER, pixel_format=RGBA8, exposure_ev=0.0,
                key_ev=F32("-2.47393119"), meter_low=0.10, meter_high=0.90, ev_min=-16.0, ev_max=16.0, adaptation=1.0, white=4.0,
                gamma=2.2, seed=0)


def lum32(rgb):
    """0.2126f*r + 0.7152f*g + 0.0722f*b, left to right, no fma"""
    rgb = np.asarray(rgb, F32)
    with np.errstate(all="ignore"):
        return (F32(0.2126) * rgb[..., 0] + F32(0.7152) * rgb[..., 1]) + F32(0.0722) * rgb[..., 2]


def bins(y):
    """the bin of each (positive, finite) luminance: clamp((int)(bits(Y) >> 20) - 888, 0, 255)"""
    bits = np.ascontiguousarray(y, F32).view(np.uint32)
    return np.clip((bits >> 20).astype(np.int64) - 888, 0, 255)


def histogram(rgb):
    """(256 uint32 counts, metered mask) of an (..., 3) float32 frame"""
    rgb = np.asarray(rgb, F32)
    y = lum32(rgb)
    metered = np.isfinite(rgb).all(axis=-1) & np.isfinite(y) & (y > 0)
    return np.bincount(bins(y[metered]), minlength=BINS).astype(np.uint32), metered


def lam(b):
    return float((b >> 3) - 16) + float(L[b & 7])


def meter(hist, meter_low, meter_high):
    """the metered mean log2 luminance (float32; NaN when nothing is metered): a loop over the bins in float64"""
    total = int(np.asarray(hist, np.uint64).sum())
    lo = math.floor(float(total) * float(F32(meter_low)))
    hi = math.ceil(float(total) * float(F32(meter_high)))
    num = den = 0.0
    c = 0
    for b in range(BINS):
        n = int(hist[b])
        o = float(max(0.0, min(float(c + n), float(hi)) - max(float(c), float(lo))))
        den = den + o
        num = num + o * lam(b)
        c += n
    return F32(num / den) if den > 0.0 else F32("nan")


def powf(O, x, y):
    x = np.ascontiguousarray(x, F32)
    return O.detmath(6, x, np.full(x.shape, y, F32))


def exposure(hist, state=None, **opts):
    """(ev, dither frame, new state (ev, frames, metered) or None)"""
    o = dict(DEFAULTS, **opts)
    metered = meter(hist, o["meter_low"], o["meter_high"])
    target = F32(o["exposure_ev"])
    if not np.isnan(metered) and o["exposure_mode"] == AUTO:
        target = F32(min(max(F32(o["key_ev"]) - metered, F32(o["ev_min"])), F32(o["ev_max"]))) + F32(o["exposure_ev"])
    ev, frame = F32(target), 0
    new = None
    if state is not None:
        prev, frame = F32(state[0]), int(state[1])
        a = F32(o["adaptation"])
        if frame > 0 and a != F32(1):
            ev = prev + a * (target - prev)
        new = (F32(ev), min(frame + 1, 0xFFFFFFFF), metered)
    return F32(ev), frame, new


# ---- Philox4x32-10 (rt_detmath.h rt_philox4x32_10), vectorised over uint32 arrays ----
def philox(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, np.uint64) & 0xFFFFFFFF for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = c[0] * np.uint64(0xD2511F53)
        p1 = c[2] * np.uint64(0xCD9E8D57)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(0xFFFFFFFF)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(0xFFFFFFFF)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def hable(x):
    A, B, Cc, D, E, Fc = F32(0.15), F32(0.50), F32(0.10), F32(0.20), F32(0.02), F32(0.30)
    CB, DE, DF, EF = Cc * B, D * E, D * Fc, E / Fc
    with np.errstate(all="ignore"):
        return (x * (A * x + CB) + DE) / (x * (A * x + B) + DF) - EF


def tone(x, tonemap, white):
    """(..., 3) float32 after the exposure -> the tone curve"""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        if tonemap == CLAMP:
            return x
        if tonemap == REINHARD:
            w2 = F32(white) * F32(white)
            y = lum32(x)
            ok = (y > 0) & np.isfinite(y)
            k = ((y * (F32(1) + y / w2)) / (F32(1) + y)) / y
            return np.where(ok[..., None], x * k[..., None], x).astype(F32)
        if tonemap == ACES:
            return (x * (F32(2.51) * x + F32(0.03))) / (x * (F32(2.43) * x + F32(0.59)) + F32(0.14))
        if tonemap == HABLE:
            return hable(x) / hable(F32(white))
    raise ValueError(tonemap)


def transfer(O, v, kind, gamma):
    v = np.asarray(v, F32)
    if kind == SRGB:
        p = powf(O, v, F32(1) / F32(2.4))
        return np.where(v <= F32(0.0031308), F32(12.92) * v, F32(1.055) * p - F32(0.055)).astype(F32)
    if kind == GAMMA:
        return powf(O, v, F32(1) / F32(gamma))
    return v


def sat(q):
    q = np.asarray(q, F32)
    out = np.zeros(q.shape, np.uint8)
    pos = q > 0
    out[pos] = np.where(q[pos] >= 255, F32(255), q[pos]).astype(np.uint8)
    return out


def dither_u(h, w, frame, seed):
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    words = philox(x, y, np.uint64(frame), np.uint64(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([(wd >> np.uint32(8)).astype(F32) * F32(2.0 ** -24) for wd in words[:3]], axis=-1)


def map_pixels(O, rgb, ev, frame, **opts):
    """(H, W, 3) float32 frame -> (H, W, 4 | 3) uint8 at exposure ev, dither frame `frame`"""
    o = dict(DEFAULTS, **opts)
    rgb = np.asarray(rgb, F32)
    h, w = rgb.shape[:2]
    s = powf(O, np.array([2.0], F32), F32(ev))[0]
    with np.errstate(all="ignore"):
        x = rgb * s
        y = tone(x, o["tonemap"], o["white"])
        v = np.fmin(np.fmax(y, F32(0)), F32(1)).astype(F32)
        t = transfer(O, v, o["transfer"], o["gamma"])
        q = o["quantiser"]
        if q == ROUND:
            b = sat(t * F32(255) + F32(0.5))
        elif q == DITHER:
            b = sat(np.floor(t * F32(255) + dither_u(h, w, frame, int(o["seed"]))))
        else:
            b = sat(t * F32(255.999))
    fmt = o["pixel_format"]
    if fmt == RGB8:
        return b
    a = np.full((h, w, 1), 255, np.uint8)
    return np.concatenate([b[..., ::-1] if fmt == BGRA8 else b, a], axis=-1)


def display(O, rgb, state=None, **opts):
    """one call: (pixels, histogram, state after (ev, frames, metered) or None).  state None = no state (NULL); (0, 0, 0) = zero state"""
    o = dict(DEFAULTS, **opts)
    hist, _ = histogram(rgb)
    ev, frame, new = exposure(hist, state, **o)
    return map_pixels(O, rgb, ev, frame, **o), hist, new
