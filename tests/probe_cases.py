"""What the light-probe tests share: the scenes (lens_cases.SCENES), the probe positions of each, and the checker's samples, computed
once per (scene, method) on the CPU oracle and shared read-only.  test_probe.py (CPU) shows on the checker alone that every
comparison of test_gpu_probe.py tests something.  torch is never imported here."""
import functools

import numpy as np

import lens_cases as LN
import probe_checker as PC
import scenes

abi = scenes.abi
F32 = np.float32
SEED, BEGIN = 7, 5
MAX_K = 13  # the passes BEGIN .. BEGIN + 12 cover (K, S) = (4, 1), (4, 2), (7, 3) and (13, 13)
FOLDS = ((4, 1), (4, 2), (7, 3), (13, 13))
METHODS = LN.METHODS
SCENES = LN.SCENES
MANY, MANY_K, MANY_S = 70, 8, 4  # 280 slots: more than one 256-lane workgroup, the last wave partly empty
built = LN.built


@functools.lru_cache(maxsize=None)
def positions(name):
    """(5, 3) f32: the camera's place (open space), a hair above the smallest sphere, inside that sphere, far outside the scene's box,
    and halfway from the camera to what it looks at"""
    sc, cam, cpu = built(name)
    spheres = [p for p in sc.prim_records if p.type == abi.RT_PRIM_SPHERE]
    assert spheres, name
    s = min(spheres, key=lambda p: p.u.sphere.radius)
    c, r = np.array(s.u.sphere.centre[:], dtype=np.float64), float(s.u.sphere.radius)
    root = cpu.nodes()[0]
    lo, hi = (np.array(root[k], dtype=np.float64) for k in ("min", "max"))
    eye, at = (np.array(cam[k], dtype=np.float64) for k in ("origin", "lookat"))
    out = np.array([eye, c + (0.0, r * (1.0 + 1e-4) + 1e-4, 0.0), c + r * np.array([0.1, 0.2, -0.1]), hi + 10.0 * (hi - lo), 0.5 * (eye + at)]).astype(F32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def many_positions(name="all_materials"):
    """(MANY, 3) f32 seeded positions in a box around the scene's objects"""
    rng = np.random.default_rng(11)
    out = rng.uniform((-3.0, 0.05, -2.0), (3.0, 3.0, 3.0), (MANY, 3)).astype(F32)
    out.setflags(write=False)
    return out


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def samples(name, method):
    """(values (MAX_K, 5, 3), directions (MAX_K, 5, 3), ray counts (MAX_K, 5)) of the passes BEGIN .. of the scene's five probes"""
    return _frozen(PC.samples(built(name)[2], positions(name), method, SEED, BEGIN, MAX_K))


@functools.lru_cache(maxsize=None)
def many_samples(method):
    return _frozen(PC.samples(built("all_materials")[2], many_positions(), method, SEED, BEGIN, MANY_K))


def reference(name, method, k, split, convolve=0):
    """(coefficients (5, 9, 3), rays_shot) of the first k passes"""
    values, dirs, rays = samples(name, method)
    return PC.project(values[:k], dirs[:k], split, convolve), int(rays[:k].sum())


def many_reference(method, convolve=0):
    values, dirs, rays = many_samples(method)
    return PC.project(values, dirs, MANY_S, convolve), int(rays.sum())


def opts(method, k, split, convolve=0, seed=SEED, begin=BEGIN):
    """the keywords of HipScene.probe_sh"""
    return dict(render_method=method, samples_per_probe=k, sample_split=split, convolve=convolve, seed=seed, sample_begin=begin)


def gauss_legendre_sphere(n_theta=4, n_phi=8):
    """(directions (n, 3) f64, weights (n,) summing to 4 pi): Gauss-Legendre in cos theta times a uniform azimuth -- exact for
    polynomials of degree 2 n_theta - 1 in z and degree n_phi - 1 in the azimuth, so for the degree-4 products of the basis"""
    z, wz = np.polynomial.legendre.leggauss(n_theta)
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    s = np.sqrt(1.0 - zz * zz)
    d = np.stack([s * np.cos(pp), s * np.sin(pp), zz], axis=-1).reshape(-1, 3)
    w = np.repeat(wz, n_phi) * (2.0 * np.pi / n_phi)
    return d, w
