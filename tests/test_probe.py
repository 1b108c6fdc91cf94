"""Light probes (rt_probe_sh, rt_probe_sh_eval) without a GPU: the struct against gcc, every status code of all entry points on a
host-only scene in the order include/rt_hip.h states, rt_probe_workspace_bytes, and the conditions that keep the GPU comparisons of
test_gpu_probe.py from being vacuous, shown on the checker (tests/probe_checker.py) alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import probe_cases as PB
import probe_checker as PC
import scenes

abi = scenes.abi
F32 = np.float32
OK, INVALID, UNSUPPORTED, NO_DEVICE = abi.RT_OK, abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE
NAIVE, MIS = abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS
SYMBOLS = ("rt_probe_opts_default", "rt_probe_workspace_bytes", "rt_probe_sh", "rt_probe_sh_device", "rt_probe_sh_eval", "rt_probe_sh_eval_device")


def test_struct_size_and_offsets_against_a_compiled_sizeof(hb, tmp_path):
    fields = [f for f, _ in abi.ProbeOpts._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){printf("size %zu\\n", sizeof(rt_probe_opts));' + "".join(
        f'printf("{f} %zu\\n", offsetof(rt_probe_opts, {f}));' for f in fields) + 'printf("version %u\\n", RT_ABI_VERSION);return 0;}'
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(scenes.ROOT, "include"), c, "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got["size"]) == C.sizeof(abi.ProbeOpts) == abi.EXPECTED_SIZES["rt_probe_opts"][1] == 48
    assert abi.EXPECTED_SIZES["rt_probe_opts"][0] is abi.ProbeOpts and int(got["version"]) == abi.RT_ABI_VERSION == 2
    for f in fields:
        assert int(got[f]) == getattr(abi.ProbeOpts, f).offset, f
    lib = hb.lib()
    for sym in SYMBOLS:
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert sum("probe_sh" in name or "rt_probe" in name for name in abi.EXPORTED_SYMBOLS) == len(SYMBOLS)


def test_defaults(hb):
    o = hb.probe_opts()
    d = abi.default_probe_opts()
    assert bytes(o) == bytes(d)
    assert (o.seed, o.sample_begin, o.samples_per_probe, o.sample_split, o.render_method, o.max_depth, o.rr_threshold, o.convolve) == (0, 0, 1024, 64, MIS, 50, 3, 0)
    assert tuple(o.reserved) == (0, 0)
    assert hb.lib().rt_probe_opts_default(None) == INVALID
    with pytest.raises(ValueError):
        hb.probe_opts(samples=3)


def test_workspace_bytes(hb):
    assert hb.probe_workspace_bytes(0) == 0
    assert hb.probe_workspace_bytes(1, samples_per_probe=1, sample_split=1) == 108
    assert hb.probe_workspace_bytes(4096) == 108 * 4096 * 64
    assert hb.probe_workspace_bytes(70, samples_per_probe=8, sample_split=4) == 108 * 280
    assert hb.HipScene.probe_workspace_bytes(3, samples_per_probe=7, sample_split=3) == 108 * 9
    assert hb.probe_workspace_bytes((1 << 31) - 1, samples_per_probe=1, sample_split=1) == 108 * ((1 << 31) - 1)
    lib, n = hb.lib(), C.c_uint64(99)
    good = hb.probe_opts()
    assert lib.rt_probe_workspace_bytes(C.c_uint64(1), None, C.byref(n)) == INVALID
    assert lib.rt_probe_workspace_bytes(C.c_uint64(1), C.byref(good), None) == INVALID
    for bad in (dict(samples_per_probe=0), dict(sample_split=0), dict(samples_per_probe=8, sample_split=9), dict(render_method=2), dict(convolve=2)):
        assert lib.rt_probe_workspace_bytes(C.c_uint64(1), C.byref(hb.probe_opts(**bad)), C.byref(n)) == INVALID, bad
    assert lib.rt_probe_workspace_bytes(C.c_uint64(1 << 25), C.byref(good), C.byref(n)) == UNSUPPORTED  # 2^25 x 64 slots
    assert lib.rt_probe_workspace_bytes(C.c_uint64((1 << 25) - 1), C.byref(good), C.byref(n)) == OK and n.value == 108 * 64 * ((1 << 25) - 1)
    assert lib.rt_probe_workspace_bytes(C.c_uint64(1 << 62), C.byref(hb.probe_opts(sample_split=4)), C.byref(n)) == UNSUPPORTED  # (the product would wrap)


def test_status_codes_without_a_device(hb):
    s = hb.HipScene(scenes.load_ssml("rtweekend1").scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    n = 5
    pos, out, work = np.full((n, 3), 7.0, F32), np.full((n, 9, 3), 7.0, F32), np.full((n * 64, 27), 7.0, F32)
    rays = C.c_uint64(99)

    def call(device, *, scene=s._h, positions=pos, n_probes=n, no_opts=False, output=out, workspace=work, reserved=0, **fields):
        o = hb.probe_opts(**fields)
        o.reserved[1] = reserved
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        head = (scene, ptr(positions), C.c_uint64(n_probes), None if no_opts else C.byref(o), ptr(output))
        if device:
            return lib.rt_probe_sh_device(*head, ptr(workspace), C.byref(rays), C.c_void_p(0))
        return lib.rt_probe_sh(*head, C.byref(rays))

    for device in (False, True):
        assert call(device) == NO_DEVICE
        for good in (dict(sample_split=1), dict(samples_per_probe=7, sample_split=7), dict(render_method=NAIVE), dict(convolve=1),
                     dict(sample_begin=(1 << 64) - 1, seed=(1 << 64) - 1), dict(samples_per_probe=(1 << 32) - 1), dict(max_depth=1, rr_threshold=0)):
            assert call(device, **good) == NO_DEVICE, good
        assert call(device, n_probes=0) == NO_DEVICE  # the device is looked at before the empty batch, as rt_radiance does
        # a host-only scene reports bad arguments as such
        assert call(device, scene=None) == INVALID
        assert call(device, positions=None) == INVALID
        assert call(device, no_opts=True) == INVALID
        assert call(device, output=None) == INVALID
        for bad in (dict(samples_per_probe=0), dict(sample_split=0), dict(samples_per_probe=8, sample_split=9), dict(render_method=2),
                    dict(render_method=-1), dict(convolve=2), dict(reserved=1)):
            assert call(device, **bad) == INVALID, bad
        # unsupported comes after the argument errors and before the device
        assert call(device, n_probes=1 << 25) == UNSUPPORTED
        assert call(device, n_probes=(1 << 25) - 1) == NO_DEVICE
        assert call(device, n_probes=1 << 31, sample_split=1) == UNSUPPORTED
        assert call(device, n_probes=1 << 25, convolve=2) == INVALID
        assert call(device, n_probes=1 << 25, reserved=1) == INVALID
    assert call(True, workspace=None) == INVALID
    assert call(True, workspace=None, n_probes=0) == INVALID
    assert call(False, workspace=None) == NO_DEVICE  # (the host form has no workspace argument)
    assert (pos == 7.0).all() and (out == 7.0).all() and (work == 7.0).all() and rays.value == 99
    with pytest.raises(hb.RtHipError) as e:
        s.probe_sh(pos, samples_per_probe=4, sample_split=2)
    assert e.value.code == NO_DEVICE


def test_eval_status_codes_without_a_device(hb):
    s = hb.HipScene(scenes.load_ssml("rtweekend1").scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    n, m = 4, 6
    co, nm, out = np.full((n, 9, 3), 7.0, F32), np.full((m, 3), 7.0, F32), np.full((m, 3), 7.0, F32)
    idx = np.array([0, 3, 1, 1, 2, 0], np.uint32)

    def call(device, *, scene=s._h, coeffs=co, n_probes=n, index=idx, normals=nm, count=m, output=out):
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        args = (scene, ptr(coeffs), C.c_uint64(n_probes), ptr(index), ptr(normals), C.c_uint64(count), ptr(output))
        return lib.rt_probe_sh_eval_device(*args, C.c_void_p(0)) if device else lib.rt_probe_sh_eval(*args)

    for device in (False, True):
        assert call(device) == NO_DEVICE
        assert call(device, count=0) == NO_DEVICE
        assert call(device, index=None, count=4) == NO_DEVICE
        assert call(device, scene=None) == INVALID
        assert call(device, coeffs=None) == INVALID
        assert call(device, normals=None) == INVALID
        assert call(device, output=None) == INVALID
    # an index past the probes: the host form refuses it, the device form cannot look (it writes NaN there)
    assert call(False, index=np.array([0, 3, 1, 4, 2, 0], np.uint32)) == INVALID
    assert call(False, index=None) == INVALID  # six normals, four probes, no list
    assert call(False, n_probes=3) == INVALID
    assert call(True, index=None) == NO_DEVICE
    assert (co == 7.0).all() and (nm == 7.0).all() and (out == 7.0).all()
    with pytest.raises(ValueError):
        s.probe_sh_eval(co, nm, idx[:5])
    with pytest.raises(hb.RtHipError) as e:
        s.probe_sh_eval(co, nm, idx)
    assert e.value.code == NO_DEVICE


# ---- what keeps the GPU comparisons from being vacuous, on the checker alone ----
def test_the_basis_is_orthonormal():
    """the Gram matrix over a quadrature that is exact for degree 4 (4 Gauss-Legendre nodes x 8 azimuths) is the identity within 1e-5:
    each of its 32 terms carries a few f32 roundings (6e-8 each) of values below 1.2"""
    d, w = PB.gauss_legendre_sphere()
    assert abs(w.sum() - 4.0 * np.pi) < 1e-12
    y = PC.basis(d.astype(F32)).astype(np.float64)
    gram = np.einsum("n,ni,nj->ij", w, y, y)
    assert np.abs(gram - np.eye(9)).max() <= 1e-5, gram


def test_every_direction_is_a_unit_vector():
    for n in (0, PB.BEGIN, (1 << 64) - 1):
        d = PC.directions(PB.SEED, range(200), n).astype(np.float64)
        assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 1e-6
    # both hemispheres, all four quadrants: a sphere, not a cap
    d = PC.directions(PB.SEED, range(200), 1)
    assert all((np.sign(d) == s).all(axis=1).any() for s in np.array(np.meshgrid([-1, 1], [-1, 1], [-1, 1])).reshape(3, -1).T)
    # another probe, another pass, another seed: other directions
    a = PC.directions(PB.SEED, [3], 5)
    assert (a != PC.directions(PB.SEED, [4], 5)).any() and (a != PC.directions(PB.SEED, [3], 6)).any() and (a != PC.directions(PB.SEED + 1, [3], 5)).any()


def test_the_positions_are_where_they_should_be():
    for name in PB.SCENES:
        sc, _, cpu = PB.built(name)
        pos = PB.positions(name).astype(np.float64)
        spheres = [p for p in sc.prim_records if p.type == abi.RT_PRIM_SPHERE]
        s = min(spheres, key=lambda p: p.u.sphere.radius)
        c, r = np.array(s.u.sphere.centre[:]), s.u.sphere.radius
        assert 0 < np.linalg.norm(pos[1] - c) - r < 1e-3 * max(1.0, r)  # a hair above
        assert np.linalg.norm(pos[2] - c) < 0.5 * r  # inside
        root = cpu.nodes()[0]
        assert (pos[3] > np.array(root["max"])).all()  # outside the scene's box


def test_two_splits_and_two_methods_give_other_bytes():
    for name in PB.SCENES:
        for method in PB.METHODS:
            a, b = PB.reference(name, method, 7, 3)[0], PB.reference(name, method, 7, 1)[0]
            assert (a.view(np.uint32) != b.view(np.uint32)).any(), (name, method)
            assert np.isfinite(a).all() or method == MIS
        naive, mis = PB.reference(name, NAIVE, 13, 13)[0], PB.reference(name, MIS, 13, 13)[0]
        # (a probe whose samples all leave into the sky is the same under both: the integrators differ from the first bounce on)
        assert (naive.view(np.uint32) != mis.view(np.uint32)).any(axis=(1, 2)).sum() >= 2, name
        # the probes differ from each other (a probe shut inside an opaque sphere, or far out under a black sky, is all zeros)
        assert len({naive[i].tobytes() for i in range(5)}) >= 3 and (naive != 0).any(axis=(1, 2)).sum() >= 2, name


def test_convolve_scales_the_bands_exactly():
    for name in PB.SCENES:
        plain, conv = PB.reference(name, MIS, 7, 3, 0)[0], PB.reference(name, MIS, 7, 3, 1)[0]
        for j, f in enumerate(PC.BAND_FACTORS):
            with np.errstate(all="ignore"):
                want = (plain[:, j] * f).astype(F32)
            same = (conv[:, j].view(np.uint32) == want.view(np.uint32)) | (np.isnan(want) & np.isnan(conv[:, j]))
            assert same.all(), (name, j)
    assert PC.BAND_FACTORS.tolist() == [PC.PI] + [F32(2.0 * np.pi / 3.0)] * 3 + [F32(np.pi / 4.0)] * 5


UNIFORM_K = 4096
UNIFORM_BOUND = 6.0 * np.sqrt(4.0 * np.pi / UNIFORM_K)  # six standard deviations: Var(4 pi Y_j) = 4 pi under the uniform sphere


def uniform_coefficients(convolve, probes=3, split=64):
    dirs = np.stack([PC.directions(PB.SEED, range(probes), n) for n in range(UNIFORM_K)])
    return PC.project(np.ones_like(dirs), dirs, split, convolve)


def test_a_uniform_sphere_of_radiance_one():
    """sample values all 1: coefficient 0 is 2 sqrt(pi) within 1e-5 relative, the others are zero within six standard deviations of
    the estimator; convolved, every normal sees the irradiance pi within the same bound times the basis it is multiplied by"""
    c = uniform_coefficients(0)
    assert np.abs(c[:, 0] / (2.0 * np.sqrt(np.pi)) - 1.0).max() <= 1e-5
    assert np.abs(c[:, 1:]).max() <= UNIFORM_BOUND
    assert np.abs(c[:, 1:]).max() > 0  # an estimate, not the exact zero
    e = uniform_coefficients(1)
    rng = np.random.default_rng(3)
    nm = rng.normal(size=(100, 3))
    nm = (nm / np.linalg.norm(nm, axis=1, keepdims=True)).astype(F32)
    got = PC.evaluate(e, nm, rng.integers(0, 3, 100))
    assert np.abs(got - np.pi).max() <= eval_bound()


def eval_bound():
    """|E(n) - pi| for coefficients within UNIFORM_BOUND of (2 sqrt(pi), 0 ...) ahead of the band factors: the band-0 term's 1e-5
    relative, then sum_j factor_j * UNIFORM_BOUND * max|Y_j| over the eight other terms"""
    ymax = np.array([0.488602512] * 3 + [1.092548431 / 2] * 2 + [0.315391565 * 2] + [1.092548431 / 2] + [0.546274215])
    return 1e-5 * np.pi + float((PC.BAND_FACTORS[1:].astype(np.float64) * UNIFORM_BOUND * ymax).sum())


def test_the_evaluation_reads_the_indexed_probe():
    c = PB.reference("all_materials", NAIVE, 13, 13)[0]
    rng = np.random.default_rng(5)
    nm = rng.normal(size=(100, 3)).astype(F32)
    idx = rng.integers(0, 5, 100).astype(np.uint32)
    a, b = PC.evaluate(c, nm, idx), PC.evaluate(c[:5], nm[:5])
    assert (a[:5].view(np.uint32) != b.view(np.uint32)).any() and np.isfinite(a).all()
    ref64 = np.einsum("mjc,mj->mc", c[idx].astype(np.float64), PC.basis(nm).astype(np.float64))
    assert np.abs(a - ref64).max() <= 1e-5 * np.abs(ref64).max()
