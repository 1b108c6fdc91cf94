"""The firefly-robust combine of include/rt_hip.h (rt_robust_opts) restated in numpy float32, written from the header text.  Every
operation is one IEEE f32 operation on arrays (numpy rounds each to f32, as the kernel does with contraction off) and every sum
runs in chunk order from +0, so the GPU is held to robust() bit for bit (tests/test_gpu_robust.py).  The chunk sums come from
tests/noise_checker.py (passes, chunk_sums); its lum and its combine are the ones the header names."""
import numpy as np

import noise_checker as N

F32 = np.float32
U32 = np.uint32
TRIM, MEDIAN, GINI = range(3)  # rt_robust_mode
NOT_FINITE = U32(0xFFFFFFFF)


def luminances(sums, n, albedo=None):
    """(S, H, W) f32: l_c = lum(sum_c / n / d), the l_c of the noise estimates"""
    d = np.fmax(np.asarray(albedo, F32), F32(1e-3)) if albedo is not None else np.ones(sums.shape[1:], F32)
    with np.errstate(all="ignore"):
        return np.stack([N.lum(sums[c] / F32(n) / d) for c in range(len(sums))]).astype(F32)


def keys(l):
    """the uint32 ordering key of every l_c: 0xFFFFFFFF if not finite, else ~b for a set sign bit, b | 0x80000000 otherwise"""
    b = np.ascontiguousarray(l, F32).view(U32)
    k = np.where(b & U32(0x80000000), ~b, b | U32(0x80000000)).astype(U32)
    return np.where(np.isfinite(l), k, NOT_FINITE).astype(U32)


def ranks(k):
    """r_c = #{ j : k_j < k_c, or k_j == k_c and j < c } along axis 0"""
    split = len(k)
    r = np.zeros(k.shape, np.int64)
    for c in range(split):
        for j in range(split):
            r[c] += (k[j] < k[c]) | ((k[j] == k[c]) & (j < c))
    return r


def gini(l, r, finite):
    """(g, G) f32 from the finite chunks in chunk order; A, B start at +0"""
    sf = finite.sum(axis=0)
    a = np.zeros(l.shape[1:], F32)
    b = np.zeros(l.shape[1:], F32)
    with np.errstate(all="ignore"):
        for c in range(len(l)):
            coef = (2 * r[c] - (sf - 1)).astype(F32)  # exact: |coef| < 128
            a = np.where(finite[c], a + coef * l[c], a).astype(F32)
            b = np.where(finite[c], b + l[c], b).astype(F32)
        big_g = (a / (sf.astype(F32) * b)).astype(F32)
        # fminf(fmaxf(G, 0), 1) with C's fmaxf -- a NaN G gives 0 -- and fmaxf(-0, +0) = +0, as the header pins it
        g = np.where(big_g > 0, np.fmin(big_g, F32(1.0)), F32(0.0)).astype(F32)
    return g, big_g


def trim_count(g, sf, mode, trim=1, gini_gain=1.0):
    tmax = np.where(sf > 0, (sf - 1) // 2, 0)
    if mode == TRIM:
        return np.minimum(int(trim), tmax)
    if mode == MEDIAN:
        return tmax
    assert mode == GINI, mode
    with np.errstate(all="ignore"):
        x = np.fmin((g * F32(gini_gain)) * tmax.astype(F32), tmax.astype(F32))
    return x.astype(np.int64)  # x is finite and >= 0: truncation is C's conversion


def robust(sums, n, albedo=None, mode=GINI, trim=1, gini_gain=1.0):
    """{"out", "mean" (H, W, 3) f32, "gini" (H, W) f32, "trimmed", "dropped" (H, W) uint8, and for the tests "ranks" (S, H, W),
    "G" (H, W) before the clamp, "kept" (S, H, W) bool} of S chunk sums (S, H, W, 3) of n passes each"""
    sums = np.asarray(sums, F32)
    split = len(sums)
    assert 2 <= split <= 64 and n >= 1 and split * n < 1 << 32, (split, n)
    l = luminances(sums, n, albedo)
    finite = np.isfinite(l)
    sf = finite.sum(axis=0).astype(np.int64)
    r = ranks(keys(l))
    g, big_g = gini(l, r, finite)
    t = trim_count(g, sf, mode, trim, gini_gain)
    kept = finite & (r >= t) & (r < sf - t)
    k = sf - 2 * t
    assert ((k >= 1) | (sf == 0)).all() and (kept.sum(axis=0) == np.where(sf > 0, k, 0)).all()
    with np.errstate(all="ignore"):
        acc = np.zeros(sums.shape[1:], F32)
        for c in range(split):
            acc = np.where(kept[c][..., None], acc + sums[c], acc).astype(F32)
        mean = N.combine(sums, split * n)
        out = acc / (k * n).astype(F32)[..., None]
        out = np.where((sf == 0)[..., None], mean, out).astype(F32)
    return {"out": out, "mean": mean, "gini": g, "trimmed": t.astype(np.uint8), "dropped": (split - sf).astype(np.uint8),
            "ranks": r, "G": big_g, "kept": kept}
