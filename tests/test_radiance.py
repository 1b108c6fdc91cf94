"""Radiance queries (rt_radiance) without a GPU: the C-ABI boundary on a host-only scene -- the struct against a compiled
sizeof / offsetof, the exported symbols, the defaults, the status code of every argument check of both entry points -- and the
output rule of tests/radiance_checker.py on hand-made samples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import radiance_checker as R
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32
INVALID, UNSUPPORTED, NO_DEVICE = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE
SYMBOLS = ("rt_radiance_opts_default", "rt_radiance", "rt_radiance_device")


# ---- the C-ABI boundary ----
def test_struct_against_a_compiled_sizeof_and_offsetof(tmp_path):
    fields = [n for n, _ in abi.RadianceOpts._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){'
           'printf("size %zu\\n", sizeof(rt_radiance_opts));'
           + "".join(f'printf("{n} %zu\\n", offsetof(rt_radiance_opts, {n}));' for n in fields)
           + 'printf("abi %u\\n", RT_ABI_VERSION); printf("key %d\\n", (int)RT_TUNE_RADIANCE_GROUPS); return 0;}')
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got["size"]) == C.sizeof(abi.RadianceOpts) == abi.EXPECTED_SIZES["rt_radiance_opts"][1] == 40
    assert abi.EXPECTED_SIZES["rt_radiance_opts"][0] is abi.RadianceOpts
    for n in fields:
        assert int(got[n]) == getattr(abi.RadianceOpts, n).offset, n
    assert fields == ["seed", "sample_begin", "samples_per_ray", "render_method", "max_depth", "rr_threshold", "reserved"]
    assert int(got["abi"]) == abi.RT_ABI_VERSION == 2  # the change is additive
    assert int(got["key"]) == abi.RT_TUNE_RADIANCE_GROUPS == 8


def test_symbols_and_defaults(hb):
    lib = hb.lib()
    for sym in SYMBOLS:
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert sum("radiance" in name for name in abi.EXPORTED_SYMBOLS) == 3
    assert lib.rt_abi_version() == 2
    o = abi.RadianceOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    assert lib.rt_radiance_opts_default(C.byref(o)) == abi.RT_OK
    assert (o.seed, o.sample_begin, o.samples_per_ray, o.render_method, o.max_depth, o.rr_threshold) == (0, 0, 1, abi.RT_METHOD_MIS, 50, 3)
    assert list(o.reserved) == [0, 0]
    assert bytes(o) == bytes(hb.radiance_opts())
    assert lib.rt_radiance_opts_default(None) == INVALID
    r = hb.radiance_opts(seed=1 << 40, sample_begin=7, samples_per_ray=5, render_method=abi.RT_METHOD_NAIVE, max_depth=8, rr_threshold=0)
    assert (r.seed, r.sample_begin, r.samples_per_ray, r.render_method, r.max_depth, r.rr_threshold) == (1 << 40, 7, 5, abi.RT_METHOD_NAIVE, 8, 0)
    with pytest.raises(ValueError):
        hb.radiance_opts(samples=4)
    assert abi.RADIANCE_OPTIONS == ("seed", "sample_begin", "samples_per_ray", "render_method", "max_depth", "rr_threshold")


def test_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    n = 5
    rays = np.zeros((n, 6), F32)
    rays[:, 5] = -1.0
    streams = np.arange(n, dtype=np.uint64)
    out = np.full((n, 3), 7.0, F32)
    p_rays, p_streams, p_out = (C.c_void_p(a.ctypes.data) for a in (rays, streams, out))

    def call(device, *, scene=s._h, rays=p_rays, streams=p_streams, n=n, opts=None, out=p_out, no_opts=False):
        o = hb.radiance_opts() if opts is None else opts
        args = (scene, rays, streams, C.c_uint64(n), None if no_opts else C.byref(o), out)
        return lib.rt_radiance_device(*args, C.c_void_p(0)) if device else lib.rt_radiance(*args)

    for device in (False, True):
        assert call(device) == NO_DEVICE
        assert call(device, streams=None) == NO_DEVICE
        for good in (dict(render_method=abi.RT_METHOD_NAIVE), dict(samples_per_ray=0xFFFFFFFF), dict(max_depth=0), dict(rr_threshold=0),
                     dict(seed=(1 << 64) - 1, sample_begin=(1 << 64) - 1)):
            assert call(device, opts=hb.radiance_opts(**good)) == NO_DEVICE, good
        # a host-only scene reports bad arguments as such
        assert call(device, scene=None) == INVALID
        assert call(device, rays=None) == INVALID
        assert call(device, out=None) == INVALID
        assert call(device, no_opts=True) == INVALID
        assert call(device, opts=hb.radiance_opts(samples_per_ray=0)) == INVALID
        for method in (-1, 2, 1 << 30):
            assert call(device, opts=hb.radiance_opts(render_method=method)) == INVALID, method
        for word in range(2):
            o = hb.radiance_opts()
            o.reserved[word] = 1
            assert call(device, opts=o) == INVALID, word
        assert call(device, n=1 << 31) == UNSUPPORTED
        assert call(device, n=(1 << 31) - 1) == NO_DEVICE  # (nothing is read before the device check)
        assert call(device, n=0) == NO_DEVICE
        assert call(device, n=0, rays=None) == INVALID
    assert (out == 7.0).all()
    # the tuning key of the refill tests
    assert lib.rt_scene_set_tuning(s._h, abi.RT_TUNE_RADIANCE_GROUPS, 1) == abi.RT_OK
    assert lib.rt_scene_set_tuning(s._h, abi.RT_TUNE_RADIANCE_GROUPS, 0) == abi.RT_OK
    assert lib.rt_scene_set_tuning(s._h, abi.RT_TUNE_RADIANCE_GROUPS, 65536) == abi.RT_OK
    for bad in (-1, 65537):
        assert lib.rt_scene_set_tuning(s._h, abi.RT_TUNE_RADIANCE_GROUPS, bad) == INVALID
    assert lib.rt_scene_set_tuning(s._h, abi.RT_TUNE_RADIANCE_GROUPS + 1, 0) == INVALID
    with pytest.raises(Exception):
        s.radiance(rays[:, :3], rays[:, 3:])
    with pytest.raises(ValueError):
        s.radiance(rays[:, :3], rays[:, 3:], streams=streams[:-1])


# ---- the checker's output rule ----
def test_output_rule_on_hand_made_samples():
    big = F32(3.0e38)
    samples = np.array([
        [[1.0, 2.0, 3.0], [0.5, 0.25, 0.125], [2.0, 4.0, 8.0]],              # plain
        [[0.1, 0.2, 0.3], [0.7, 1e-8, 1e8], [0.2, 0.1, -1e8]],               # f32 rounding, order matters
        [[1.0, np.nan, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, -0.0]],             # a NaN stays one; zeros sum from +0
        [[np.inf, big, -np.inf], [1.0, big, np.inf], [1.0, 1.0, 1.0]],       # an infinity; an overflow in f32 only; inf - inf
    ], dtype=F32)
    got = R.fold_f32(samples)
    assert got.dtype == F32 and got.shape == (4, 3)
    assert got[0].tolist() == [float(F32(3.5) / F32(3.0)), float(F32(6.25) / F32(3.0)), float(F32(11.125) / F32(3.0))]
    # row 1 by hand: the sums in order, in f32
    x = F32(F32(F32(0.0) + F32(0.1)) + F32(0.7)) + F32(0.2)
    y = F32(F32(F32(0.0) + F32(0.2)) + F32(1e-8)) + F32(0.1)
    z = F32(F32(F32(0.0) + F32(0.3)) + F32(1e8)) + F32(-1e8)
    assert got[1].tolist() == [float(F32(x) / F32(3.0)), float(F32(y) / F32(3.0)), float(F32(z) / F32(3.0))]
    assert float(z) == 0.0  # 0.3 is lost beside 1e8: the order of the sum is part of the rule
    assert got[2, 0] == 1.0 and np.isnan(got[2, 1]) and got[2, 2] == 0.0 and not np.signbit(got[2, 2])
    assert got[3, 0] == np.inf and got[3, 1] == np.inf and np.isnan(got[3, 2])
    # K = 1: the sample itself
    one = R.fold_f32(samples[:, :1, :])
    assert np.array_equal(one, samples[:, 0, :], equal_nan=True)

    pre = R.fold_prefix(samples)
    assert pre.dtype == np.float64 and pre.shape == (4, 3, 3)
    assert pre[0, 0].tolist() == [1.0, 2.0, 3.0] and pre[0, 1].tolist() == [0.75, 1.125, 1.5625]
    assert pre[0, 2].tolist() == [3.5 / 3.0, 6.25 / 3.0, 11.125 / 3.0]
    # f64 keeps what f32 lost
    assert pre[1, 2, 2] == ((0.0 + float(F32(0.3))) + 1e8 + -1e8) / 3.0 != 0.0
    assert np.isnan(pre[2, :, 1]).all() and pre[2, 2, 0] == 1.0
    assert pre[3, 0, 0] == np.inf and pre[3, 1, 1] == (float(big) + float(big)) / 2.0 and np.isfinite(pre[3, 1, 1])
    assert pre[3, 0, 2] == -np.inf and np.isnan(pre[3, 1, 2]) and np.isnan(pre[3, 2, 2])
    R.assert_same_f64(pre, pre.copy(), "itself")
    with pytest.raises(AssertionError):
        R.assert_same_f64(pre, np.nextafter(pre, np.inf), "one ulp")


def test_prefix_means_and_the_ray_sets_on_the_oracle():
    """the shapes and dtypes the GPU tests rely on, and that the m = 1 mean is one f32 sample"""
    import oracle as O
    O.build()
    ls = scenes.load_ssml("overshadowed")
    cpu = O.Scene(ls.scene)
    o, d = R.pixel_centre_rays(O.camera_new(**ls.camera_params), 8, 5)
    assert o.shape == d.shape == (40, 3) and o.dtype == d.dtype == F32
    means = R.prefix_means(cpu, o, d, abi.RT_METHOD_MIS, 3, seed=5)
    assert means.shape == (40, 3, 3) and np.isfinite(means).all()
    first = means[:, 0].astype(F32)
    assert np.array_equal(first.astype(np.float64), means[:, 0])  # one sample: an f32 widened, exactly
    assert np.array_equal(R.fold_prefix(first[:, None, :])[:, 0], means[:, 0])
    assert (means[:, 0] != means[:, 1]).any()  # the samples differ: the streams do
    po, pd = R.surface_probes(cpu, o, d, seed=1)
    assert len(po) == len(pd) > 0 and po.dtype == pd.dtype == F32
