"""The light probes of include/rt_hip.h (rt_probe_sh, rt_probe_sh_eval) restated in numpy float32, written from the header text.

Every operation is one IEEE f32 operation on arrays (numpy rounds each to f32, as the kernels do with contraction off), sines and
cosines are the oracle's rt_sinf / rt_cosf (oracle.detmath), the square root numpy's (correctly rounded).  The two draws of the
probe's stream (seed, 2^63 + probe, pass) come from oracle.rng_f32.  A sample's value and its ray count are the oracle's fixed-ray
integrator on the sample's ray on the stream (seed, probe, pass) with one sample: no arithmetic of a path is restated here.  The fold
is rt_render_opts' (noise_checker.chunk_bounds gives the chunks).

  directions(seed, probes, n)            [len(probes), 3] f32: the direction of pass n (an absolute sample index) of each probe index
  basis(d)                               [..., 9] f32: Y_0 .. Y_8 on the vectors d [..., 3] as given
  samples(cpu, positions, ...)           (values (K, n, 3), directions (K, n, 3), ray counts (K, n)) of passes begin .. begin + K - 1
  project(values, dirs, split, convolve) coefficients (n, 9, 3)
  evaluate(coeffs, normals, index)       colours (m, 3)
"""
import numpy as np

import noise_checker as N

F32 = np.float32
PI, TAU = F32(3.14159274101257324219), F32(6.28318548202514648438)
PROBE_STREAM = 1 << 63
MASK64 = (1 << 64) - 1
C0, C1, C2, C20, C22 = F32(0.282094792), F32(0.488602512), F32(1.092548431), F32(0.315391565), F32(0.546274215)
FOUR_PI = F32(12.5663706)
BAND_FACTORS = np.array([PI] + [F32(2.09439510)] * 3 + [F32(0.785398163)] * 5, dtype=F32)


def directions(seed, probes, n):
    """z = 1 - 2 xi1, s = sqrt(1 - z z), phi = 2 pi xi2, d = (s cos phi, s sin phi, z) of the draws xi1, xi2 of each probe's stream"""
    import oracle as O
    xi = np.stack([O.rng_f32(seed, (PROBE_STREAM + int(i)) & MASK64, n & MASK64, 2) for i in probes]).astype(F32)
    z = (F32(1.0) - F32(2.0) * xi[:, 0]).astype(F32)
    s = np.sqrt((F32(1.0) - z * z).astype(F32)).astype(F32)
    phi = np.ascontiguousarray((TAU * xi[:, 1]).astype(F32))
    d = np.stack([s * O.detmath(1, phi), s * O.detmath(0, phi), z], axis=1).astype(F32)
    assert d.dtype == F32
    return d


def basis(d):
    d = np.asarray(d)
    assert d.dtype == F32 and d.shape[-1] == 3
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    one, three = F32(1.0), F32(3.0)
    with np.errstate(all="ignore"):
        out = np.stack([np.full(x.shape, C0, F32), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C20 * (three * (z * z) - one), C2 * (x * z),
                        C22 * (x * x - y * y)], axis=-1)
    assert out.dtype == F32
    return out


def samples(cpu, positions, method, seed, begin, k, max_depth=50, rr_threshold=3):
    """passes begin .. begin + k - 1 (mod 2^64) of the probes at `positions` (n, 3): the integrator's values (k, n, 3) f32, the
    directions (k, n, 3) f32 and the integrator's ray counts (k, n) uint64"""
    pos = np.asarray(positions, dtype=F32).reshape(-1, 3)
    n = len(pos)
    values, dirs, rays = np.zeros((k, n, 3), F32), np.zeros((k, n, 3), F32), np.zeros((k, n), np.uint64)
    for j in range(k):
        p = (begin + j) & MASK64
        dirs[j] = directions(seed, range(n), p)
        for i in range(n):
            v, rays[j, i] = cpu.integrate_ray(pos[i], dirs[j, i], method, n_samples=1, seed=seed, max_depth=max_depth, rr_threshold=rr_threshold,
                                              n_threads=1, stream=i, sample_begin=p, return_rays=True)
            values[j, i] = v.astype(F32)  # (the f64 mean of one f32 sample is that sample)
    return values, dirs, rays


def project(values, dirs, split, convolve=0):
    """(n, 9, 3) f32: per chunk from +0 in pass order acc[j][ch] += value[ch] * Y_j, the chunk sums added in chunk order from +0, times
    (4 pi / K), then the band factors"""
    values, dirs = np.asarray(values), np.asarray(dirs)
    assert values.dtype == F32 and dirs.dtype == F32 and values.shape == dirs.shape
    k, n = values.shape[:2]
    bounds = N.chunk_bounds(k, split)
    with np.errstate(all="ignore"):
        total = np.zeros((n, 9, 3), F32)
        for lo, hi in zip(bounds, bounds[1:]):
            acc = np.zeros((n, 9, 3), F32)
            for p in range(lo, hi):
                acc = (acc + (values[p][:, None, :] * basis(dirs[p])[:, :, None]).astype(F32)).astype(F32)
            total = (total + acc).astype(F32)
        out = (total * (FOUR_PI / F32(k))).astype(F32)
        if convolve:
            out = (out * BAND_FACTORS[None, :, None]).astype(F32)
    return out


def evaluate(coeffs, normals, index=None):
    """(m, 3) f32: the nine terms coeffs[p][j][ch] * Y_j(normal) added from +0 in order; p = index[i], or i"""
    coeffs, normals = np.asarray(coeffs), np.asarray(normals)
    assert coeffs.dtype == F32 and normals.dtype == F32
    c = coeffs[np.arange(len(normals)) if index is None else np.asarray(index)]
    y = basis(normals)
    with np.errstate(all="ignore"):
        out = np.zeros((len(normals), 3), F32)
        for j in range(9):
            out = (out + (c[:, j, :] * y[:, j, None]).astype(F32)).astype(F32)
    return out
