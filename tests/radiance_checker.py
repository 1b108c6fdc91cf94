"""CPU reference for the radiance queries (rt_radiance, include/rt_hip.h): the oracle's fixed-ray integrator plus the output rule.

The oracle's `integrate_ray` is Integrator::get_colour on one ray on the streams (seed, stream, sample_begin + k), k = 0 .. m-1
(by default stream 0 from sample 0), and returns the f64 mean of the m f32 samples: sequential f64 adds from 0.0, then / m.  A
query with the same stream, sample_begin + k and one sample a ray returns sample k itself, so the f64 prefix means of the GPU's
samples must EQUAL the oracle's for every m: the f32 -> f64 conversion is exact and the adds are the same adds.  No sample is
ever taken apart here; there is no new arithmetic to trust.

  prefix_means   per ray the oracle's means for m = 1 .. K
  fold_f32       the output rule of rt_radiance: per-sample f32 triples summed in order from +0, divided by K once
  fold_prefix    the f64 prefix means the oracle would return for those samples
  pixel_centre_rays / surface_probes   the two ray sets of the GPU tests
  samples / assert_matches             what the GPU test files do with a scene on the GPU (`gpu`: a HipScene; torch is not needed)
"""
import numpy as np

f32 = np.float32


def prefix_means(cpu, origins, directions, method, k, *, seed, max_depth=50, rr_threshold=3, streams=None, sample_begin=0):
    """[n, k, 3] f64: entry [i, m-1] is oracle.Scene.integrate_ray of ray i over m samples: stream streams[i] (None: 0 for every
    ray), samples sample_begin .. sample_begin + m - 1 (mod 2^64)"""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    st = np.zeros(o.shape[0], dtype=np.uint64) if streams is None else np.asarray(streams, dtype=np.uint64)
    assert st.shape == (o.shape[0],), st.shape
    out = np.zeros((o.shape[0], k, 3), dtype=np.float64)
    for i in range(o.shape[0]):
        for m in range(1, k + 1):
            out[i, m - 1] = cpu.integrate_ray(o[i], d[i], method, n_samples=m, seed=seed, max_depth=max_depth,
                                              rr_threshold=rr_threshold, n_threads=1, stream=int(st[i]), sample_begin=int(sample_begin))
    return out


def fold_f32(samples):
    """samples [n, K, 3] f32 -> [n, 3] f32: ((+0 + c0) + c1 + ...) / (float)K, every step an f32 operation"""
    s = np.asarray(samples)
    assert s.dtype == np.float32 and s.ndim == 3 and s.shape[2] == 3
    acc = np.zeros((s.shape[0], 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(s.shape[1]):
            acc = (acc + s[:, k, :]).astype(np.float32)
        return (acc / f32(s.shape[1])).astype(np.float32)


def fold_prefix(samples):
    """samples [n, K, 3] f32 -> [n, K, 3] f64: entry [i, m-1] = (0.0 + c0 + ... + c(m-1) in f64, in order) / m"""
    s = np.asarray(samples)
    assert s.dtype == np.float32 and s.ndim == 3 and s.shape[2] == 3
    out = np.zeros(s.shape, dtype=np.float64)
    for i in range(s.shape[0]):
        acc = [0.0, 0.0, 0.0]
        for m in range(s.shape[1]):
            for j in range(3):
                acc[j] = acc[j] + float(s[i, m, j])  # python floats: f64 adds, one at a time
                out[i, m, j] = acc[j] / float(m + 1) if acc[j] == acc[j] else acc[j]
    return out


def assert_same_f64(got, ref, what):
    """every f64 equal by value, any NaN equal to any NaN (zeros of either sign are equal: a mean does not keep the sign)"""
    a, b = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    if not same.all():
        bad = np.argwhere(~same)
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: gpu {a[tuple(bad[0])]!r} oracle {b[tuple(bad[0])]!r}")


def pixel_centre_rays(camera, width, height):
    """(origins [n, 3], un-normalised directions [n, 3]) f32 through the centres of a width x height grid, row-major, y down:
    SimpleCamera::get_ray's expression with (x + 0.5, y + 0.5) in place of the jittered position"""
    x, y = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(height, dtype=np.float32))
    u = ((x.reshape(-1) + f32(0.5)) / f32(width - 1)).astype(np.float32)
    v = (f32(1.0) - (y.reshape(-1) + f32(0.5)) / f32(height - 1)).astype(np.float32)
    o = np.array(camera.origin[:], dtype=np.float32)
    ll = np.array(camera.lower_left[:], dtype=np.float32)
    hz = np.array(camera.horizontal[:], dtype=np.float32)
    vt = np.array(camera.vertical[:], dtype=np.float32)
    d = ((ll[None, :] + hz[None, :] * u[:, None]) + vt[None, :] * v[:, None]) - o[None, :]
    return np.broadcast_to(o, d.shape).copy(), d.astype(np.float32)


def surface_probes(cpu, origins, directions, seed):
    """for every ray that hits something: origin = hit point + 1e-3 * normal, direction = a seeded random direction in the
    normal's hemisphere (a normal with a non-finite component gives no probe)"""
    rec = cpu.check_hit(origins, directions)
    hit = (rec["found"] != 0) & (rec["index"] != np.uint64(0xFFFFFFFFFFFFFFFF))
    hit &= np.isfinite(rec["normal"]).all(axis=1) & np.isfinite(rec["point"]).all(axis=1)
    p, n = rec["point"][hit].astype(np.float32), rec["normal"][hit].astype(np.float32)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=p.shape).astype(np.float32)
    flip = (d * n).sum(axis=1) < 0
    d[flip] = -d[flip]
    return (p + f32(1e-3) * n).astype(np.float32), d


def samples(gpu, o, d, method, k, seed, *, streams=None, sample_begin=0, **kw):
    """[n, k, 3] f32: sample j of every ray on its stream (None: stream 0 for every ray) at sample_begin + j (mod 2^64), one query
    a sample"""
    st = np.zeros(len(o), dtype=np.uint64) if streams is None else streams
    return np.stack([gpu.radiance(o, d, streams=st, method=method, samples=1, seed=seed, sample_begin=(sample_begin + j) & ((1 << 64) - 1), **kw)
                     for j in range(k)], axis=1)


def assert_matches(gpu, o, d, ref, method, seed, what, *, streams=None, sample_begin=0, **kw):
    """the f64 prefix means of the GPU's samples EQUAL `ref` ([n, k, 3] from prefix_means at the same arguments); returns the samples"""
    got = samples(gpu, o, d, method, ref.shape[1], seed, streams=streams, sample_begin=sample_begin, **kw)
    assert_same_f64(fold_prefix(got), ref, what)
    return got
