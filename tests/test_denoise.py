"""The A-Trous denoiser (rt_denoise, include/rt_hip.h) without a GPU: the numpy checker (tests/denoise_checker.py) pinned to
independent constructions, and the ABI surface and status codes of the entry points on a host-only scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_checker as K
import scenes

abi = scenes.abi
ROOT = scenes.ROOT


# ---- the checker ----
def test_constant_image_stays_constant():
    c = np.full((11, 13, 3), (0.3, 0.5, 0.7), np.float32)
    for it in (1, 5):
        assert np.allclose(K.denoise(c, iterations=it), c, rtol=1e-12, atol=0)


def test_one_iteration_is_the_b3_spline_with_huge_variance():
    """no guides, a variance so large that w_l -> 1: one iteration is the 5 x 5 B3-spline convolution, renormalised over the
    taps inside the frame"""
    rng = np.random.default_rng(1)
    h, w = 9, 12
    c = rng.uniform(0.1, 1.0, (h, w, 3)).astype(np.float32)
    var = np.full((h, w), 1e30, np.float32)
    got = K.denoise(c, variance=var, iterations=1)
    k1 = np.array([1, 4, 6, 4, 1], np.float64) / 16
    ref = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            num, den = np.zeros(3), 0.0
            for j in range(5):
                for i in range(5):
                    yy, xx = y + j - 2, x + i - 2
                    if 0 <= yy < h and 0 <= xx < w:
                        num += k1[j] * k1[i] * c[yy, xx]
                        den += k1[j] * k1[i]
            ref[y, x] = num / den
    assert np.allclose(got, ref, rtol=1e-12, atol=1e-12)


def _half_planes(h=16, w=20):
    c = np.zeros((h, w, 3), np.float32)
    c[:, : w // 2] = (0.9, 0.2, 0.1)
    c[:, w // 2:] = (0.1, 0.3, 0.8)
    return c


def test_half_planes_do_not_bleed():
    h, w = 16, 20
    c = _half_planes(h, w)
    var = np.full((h, w), 1e30, np.float32)  # the luminance weight alone would mix them
    normal = np.zeros((h, w, 3), np.float32)
    normal[:, : w // 2] = (1, 0, 0)
    normal[:, w // 2:] = (0, 1, 0)
    depth = np.zeros((h, w), np.float32)
    depth[:, w // 2:] = 5.0
    assert K.relative_error(K.denoise(c, normal=normal, variance=var), c) < 1e-12
    assert K.relative_error(K.denoise(c, depth=depth, variance=var), c) < 1e-12
    assert K.relative_error(K.denoise(c, variance=var), c) > 0.1  # without a guide they do mix


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("with_variance", [False, True])
def test_invalid_pixel_passes_through_and_is_not_a_tap(bad, with_variance):
    rng = np.random.default_rng(2)
    h, w = 12, 14
    c = rng.uniform(0.1, 1.0, (h, w, 3)).astype(np.float32)
    var = rng.uniform(0.0, 0.05, (h, w)).astype(np.float32) if with_variance else None
    normal = rng.normal(size=(h, w, 3)).astype(np.float32)
    depth = rng.uniform(1, 2, (h, w)).astype(np.float32)
    poisoned = c.copy()
    poisoned[5, 6, 1] = bad
    exclude = np.zeros((h, w), bool)
    exclude[5, 6] = True
    got = K.denoise(poisoned, normal=normal, depth=depth, variance=var)
    masked = K.denoise(c, normal=normal, depth=depth, variance=var, exclude=exclude)
    plain = K.denoise(c, normal=normal, depth=depth, variance=var)
    assert np.array_equal(got[5, 6], poisoned[5, 6].astype(np.float64), equal_nan=True)
    keep = ~exclude
    assert np.isfinite(got[keep]).all()
    assert np.array_equal(got[keep], masked[keep])
    assert not np.allclose(got[keep], plain[keep])  # the pixel was a tap of its neighbours before


def test_invalid_variance_marks_the_pixel():
    c = np.full((6, 7, 3), 0.5, np.float32)
    c[2, 3] = 9.0
    var = np.full((6, 7), 0.01, np.float32)
    var[2, 3] = np.nan
    got = K.denoise(c, variance=var)
    assert np.array_equal(got[2, 3], c[2, 3])
    assert np.allclose(np.delete(got.reshape(-1, 3), 2 * 7 + 3, axis=0), 0.5, rtol=1e-12)


def test_spatial_variance_is_the_two_pass_box():
    rng = np.random.default_rng(3)
    c = rng.uniform(0, 1, (7, 8, 3)).astype(np.float32)
    _, e, var, valid, _, _ = K.prepare(c)
    l = K.lum(e)
    for y, x in ((0, 0), (3, 4), (6, 7), (2, 7)):
        box = l[max(0, y - 2):y + 3, max(0, x - 2):x + 3].ravel()
        assert np.isclose(var[y, x], np.mean((box - box.mean()) ** 2), rtol=1e-12)


def test_halves_variance_formula():
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 2, (5, 6, 3)).astype(np.float32)
    b = rng.uniform(0, 2, (5, 6, 3)).astype(np.float32)
    alb = rng.uniform(0, 1, (5, 6, 3)).astype(np.float32)
    alb[0, 0] = 0.0  # the 1e-3 floor
    got = K.halves_variance(a, b, alb)
    assert got.dtype == np.float32
    d = np.maximum(alb.astype(np.float64), float(np.float32(1e-3)))
    la, lb = K.lum(a / d), K.lum(b / d)
    assert np.allclose(got, (la - lb) ** 2 / 4, rtol=1e-5, atol=1e-9)
    # with identical halves the variance is exactly 0
    assert not K.halves_variance(a, a, alb).any()


# ---- the library without a device ----
def _inputs(h, w, which=("color", "albedo", "normal", "depth", "variance")):
    ins, keep = abi.DenoiseInputs(), []
    for name in which:
        a = np.zeros((h, w, 3) if name in ("color", "albedo", "normal") else (h, w), np.float32)
        keep.append(a)
        setattr(ins, name, a.ctypes.data_as(C.POINTER(C.c_float)))
    return ins, keep


def test_denoise_symbols_and_structs(hb):
    lib = hb.lib()
    for sym in ("rt_denoise_opts_default", "rt_denoise_workspace_bytes", "rt_denoise", "rt_denoise_device", "rt_render_denoised"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(abi.DenoiseOpts) == abi.EXPECTED_SIZES["rt_denoise_opts"][1] == 48
    assert C.sizeof(abi.DenoiseInputs) == abi.EXPECTED_SIZES["rt_denoise_inputs"][1] == 40
    assert tuple(n for n, _ in abi.DenoiseInputs._fields_) == abi.DENOISE_INPUTS


def test_opts_default(hb):
    o = abi.DenoiseOpts()
    o.width, o.height, o.reserved[2] = 7, 9, 5
    assert hb.lib().rt_denoise_opts_default(C.byref(o)) == abi.RT_OK
    assert (o.width, o.height, o.iterations) == (0, 0, 5)
    assert (o.sigma_luminance, o.sigma_normal) == (4.0, 128.0)
    assert o.sigma_depth == np.float32(0.1)
    assert list(o.reserved) == [0] * 6
    assert hb.lib().rt_denoise_opts_default(None) == abi.RT_ERR_INVALID_ARGUMENT
    p = hb.denoise_opts(3, 4, iterations=2)
    assert (p.width, p.height, p.iterations, p.sigma_normal) == (3, 4, 2, 128.0)


@pytest.mark.parametrize("w,h", [(1, 1), (64, 36), (67, 37), (1920, 1080), (1 << 16, 1 << 15)])
def test_workspace_bytes(hb, w, h):
    assert hb.denoise_workspace_bytes(hb.denoise_opts(w, h)) == 48 * w * h


def test_workspace_bytes_rejects(hb):
    lib = hb.lib()
    n = C.c_uint64()
    assert lib.rt_denoise_workspace_bytes(C.byref(hb.denoise_opts(0, 5)), C.byref(n)) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_denoise_workspace_bytes(C.byref(hb.denoise_opts(1 << 16, (1 << 15) + 1)), C.byref(n)) == abi.RT_ERR_UNSUPPORTED
    assert lib.rt_denoise_workspace_bytes(None, C.byref(n)) == abi.RT_ERR_INVALID_ARGUMENT


def _expect(lib, rc, code, words):
    assert rc == code, (rc, code, lib.rt_last_error())
    msg = lib.rt_last_error().decode()
    assert all(word in msg for word in words), msg


def test_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    h, w = 9, 16
    ins, _keep = _inputs(h, w)
    out = np.zeros((h, w, 3), np.float32)
    ws = np.zeros(48 * w * h // 4 + 4, np.float32)
    ws_ptr = C.c_void_p((ws.ctypes.data + 15) // 16 * 16)
    out_p = out.ctypes.data_as(C.POINTER(C.c_float))

    def call(inputs, opts, out_ptr, device, workspace=ws_ptr):
        if device:
            return lib.rt_denoise_device(s._h, C.byref(inputs), C.byref(opts), workspace, out_ptr, C.c_void_p(0))
        return lib.rt_denoise(s._h, C.byref(inputs), C.byref(opts), out_ptr)

    inv, uns = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED
    for device in (False, True):
        good = hb.denoise_opts(w, h)
        _expect(lib, call(ins, good, out_p, device), abi.RT_ERR_NO_DEVICE, ["host-only"])
        for which in (("color",), ("color", "albedo"), ("color", "normal", "depth")):
            _expect(lib, call(_inputs(h, w, which)[0], good, out_p, device), abi.RT_ERR_NO_DEVICE, ["host-only"])
        no_color, _k = _inputs(h, w, ("albedo", "normal"))
        _expect(lib, call(no_color, good, out_p, device), inv, ["color"])
        _expect(lib, call(ins, good, None, device), inv, ["out"])
        for name in abi.DENOISE_INPUTS:  # out aliasing an input
            _expect(lib, call(ins, good, C.cast(getattr(ins, name), C.POINTER(C.c_float)), device), inv, ["overlaps"])
        for ww, hh in ((0, h), (w, 0)):
            _expect(lib, call(ins, hb.denoise_opts(ww, hh), out_p, device), inv, ["width"])
        for it in (0, 11):
            _expect(lib, call(ins, hb.denoise_opts(w, h, iterations=it), out_p, device), inv, ["iterations"])
        for key in ("sigma_luminance", "sigma_normal", "sigma_depth"):
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                _expect(lib, call(ins, hb.denoise_opts(w, h, **{key: bad}), out_p, device), inv, ["sigma"])
        _expect(lib, call(ins, hb.denoise_opts(1 << 16, (1 << 15) + 1), out_p, device), uns, ["2^31"])
        assert lib.rt_denoise(None, C.byref(ins), C.byref(good), out_p) == inv
    # the device call's workspace: NULL, misaligned, overlapping
    good = hb.denoise_opts(w, h)
    _expect(lib, call(ins, good, out_p, True, None), inv, ["workspace"])
    _expect(lib, call(ins, good, out_p, True, C.c_void_p(ws_ptr.value + 4)), inv, ["workspace"])
    _expect(lib, call(ins, good, out_p, True, C.c_void_p(out.ctypes.data)), inv, ["workspace"])
    with pytest.raises(hb.RtHipError) as e:
        s.denoise(out)
    assert e.value.code == abi.RT_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        s.denoise(out, depth=np.zeros((h + 1, w), np.float32))


def test_render_denoised_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    cam = hb.camera_new(**ls.camera_params)
    lib = hb.lib()
    w, h = 16, 9
    clean = np.zeros((h, w, 3), np.float32)
    noisy = np.zeros((h, w, 3), np.float32)
    cp, np_ = clean.ctypes.data_as(C.POINTER(C.c_float)), noisy.ctypes.data_as(C.POINTER(C.c_float))
    rays = C.c_uint64()

    def call(opts, dopts, clean_ptr=cp, noisy_ptr=np_):
        return lib.rt_render_denoised(s._h, C.byref(cam), C.byref(opts), C.byref(dopts), clean_ptr, noisy_ptr, C.byref(rays))

    dn = hb.denoise_opts(0, 0)  # its width and height are ignored
    inv, uns = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED
    _expect(lib, call(abi.default_render_opts(w, h, 4), dn), abi.RT_ERR_NO_DEVICE, ["host-only"])
    _expect(lib, call(abi.default_render_opts(w, h, 4), dn, noisy_ptr=None), abi.RT_ERR_NO_DEVICE, ["host-only"])
    for spp in (0, 1, 3, 7):
        _expect(lib, call(abi.default_render_opts(w, h, spp), dn), inv, ["samples_per_pixel"])
    _expect(lib, call(abi.default_render_opts(w, h, 4), dn, clean_ptr=None), inv, ["null"])
    _expect(lib, call(abi.default_render_opts(w, h, 4), dn, noisy_ptr=cp), inv, ["overlaps"])
    for ww, hh in ((0, h), (w, 0)):
        _expect(lib, call(abi.default_render_opts(ww, hh, 4), dn), inv, ["width"])
    _expect(lib, call(abi.default_render_opts(w, h, 4), hb.denoise_opts(0, 0, iterations=11)), inv, ["iterations"])
    _expect(lib, call(abi.default_render_opts(w, h, 4), hb.denoise_opts(0, 0, sigma_depth=-1.0)), inv, ["sigma"])
    o = abi.default_render_opts(w, h, 4)
    o.output_layout = abi.RT_LAYOUT_SHARD
    _expect(lib, call(o, dn), uns, ["FRAME"])
    o = abi.default_render_opts(w, h, 4)
    o.shard_count = 2
    _expect(lib, call(o, dn), uns, ["shard_count"])
    _expect(lib, call(abi.default_render_opts(1 << 16, (1 << 15) + 1, 4), dn), uns, ["2^31"])
    with pytest.raises(hb.RtHipError) as e:
        s.render_denoised(cam, abi.default_render_opts(w, h, 4))
    assert e.value.code == abi.RT_ERR_NO_DEVICE


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() {\n'
           'std::vector<float> (*f)(const rt_hip::Bvh &, const std::vector<float> &, const rt_hip::AovBuffers *, uint32_t, uint32_t,'
           ' const rt_hip::DenoiseOptions &) = &rt_hip::denoise;\n'
           'rt_hip::Denoised (*g)(const rt_hip::RenderOptions &, const rt_hip::SimpleCamera &, const rt_hip::Bvh &,'
           ' const rt_hip::DenoiseOptions &, uint64_t, uint64_t) = &rt_hip::render_denoised;\n'
           '(void)f; (void)g; return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)
