"""The display stage (rt_display, include/rt_hip.h) without a GPU: the numpy checker (tests/display_checker.py) on analytic cases,
auto-exposure of a committed fixture, and the ABI surface and status codes on a host-only scene."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import display_checker as D
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32


def gray(h, w, v):
    return np.full((h, w, 3), v, F32)


# ---- the checker on analytic cases ----
def test_bin_edges_at_powers_of_two():
    for k in range(-16, 16):
        v = F32(2.0 ** k)
        assert D.bins(np.array([v]))[0] == 8 * (k + 16), k
        below = np.nextafter(v, F32(0))
        assert D.bins(np.array([below]))[0] == max(0, 8 * (k + 16) - 1), k
        for m in range(8):  # sub-bin m of the octave starts at 2^k * (1 + m/8)
            assert D.bins(np.array([F32(2.0 ** k * (1 + m / 8))]))[0] == 8 * (k + 16) + m
    assert D.bins(np.array([F32(2.0 ** -16)]))[0] == 0
    assert D.bins(np.array([F32(2.0 ** 16)]))[0] == 255
    assert list(D.bins(np.array([F32(1e-30), F32(1e30), F32(2.0 ** 16 - 1)], F32))) == [0, 255, 255]


def test_log2_literals():
    for m in range(8):
        assert D.L[m] == F32(math.log2(1 + (m + 0.5) / 8)), m
    assert D.DEFAULTS["key_ev"] == F32(math.log2(0.18))


def test_unmetered_pixels():
    img = gray(4, 8, 0.5)
    img[0, 0] = (np.nan, 0.5, 0.5)
    img[0, 1] = (np.inf, 0.5, 0.5)
    img[0, 2] = (0.0, 0.0, 0.0)
    img[0, 3] = (-1.0, -1.0, -1.0)
    img[0, 4] = (1.0, -1.0, 0.0)    # Y < 0
    img[0, 5] = (-np.inf, 0.0, 0.0)
    img[0, 6] = (3e38, 3e38, 3e38)  # huge but finite: metered, in the top bin
    hist, metered = D.histogram(img)
    assert hist.sum() == 32 - 6 and not metered[0, :6].any() and metered[0, 6:].all() and metered[1:].all()
    assert hist[D.bins(D.lum32(img[1:2, 0]))[0]] == 25 and hist[255] == 1


def test_constant_image_meters_its_own_bin():
    for v in (0.3, 0.0065, 1.0, 77.0):
        img = gray(9, 16, v)
        hist, _ = D.histogram(img)
        b = int(D.bins(D.lum32(img[:1, 0]))[0])
        assert hist[b] == 144
        assert D.meter(hist, 0.1, 0.9) == F32(D.lam(b))
        ev, frame, new = D.exposure(hist, exposure_mode=D.AUTO)
        assert ev == F32(D.DEFAULTS["key_ev"]) - F32(D.lam(b)) and frame == 0 and new is None


def test_two_level_image_percentile_clipping():
    img = gray(10, 10, 0.25)
    img[0, :5] = 64.0  # 5 % of the pixels, far brighter
    hist, _ = D.histogram(img)
    b_dim, b_bright = int(D.bins(D.lum32(img[1:2, 0]))[0]), int(D.bins(D.lum32(img[0:1, 0]))[0])
    assert D.meter(hist, 0.10, 0.90) == F32(D.lam(b_dim))  # the bright 5 % lie above the 90th percentile
    everything = D.meter(hist, 0.0, 1.0)
    assert everything == F32((95 * D.lam(b_dim) + 5 * D.lam(b_bright)) / 100)
    assert D.meter(hist, 0.97, 1.0) == F32(D.lam(b_bright))
    # an empty histogram meters nothing: the target is exposure_ev
    empty = np.zeros(256, np.uint32)
    assert np.isnan(D.meter(empty, 0.1, 0.9))
    assert D.exposure(empty, exposure_ev=1.5)[0] == F32(1.5)


def test_adaptation_converges_geometrically():
    bright, dim = D.histogram(gray(8, 8, 4.0))[0], D.histogram(gray(8, 8, 0.05))[0]
    state = (F32(0), 0, F32(0))
    ev0, frame, state = D.exposure(bright, state, adaptation=0.3)  # frames == 0: snaps
    assert frame == 0 and ev0 == D.exposure(bright)[0] and state[1] == 1
    target = D.exposure(dim)[0]
    for k in range(1, 12):
        ev, frame, state = D.exposure(dim, state, adaptation=0.3)
        assert frame == k and state[1] == k + 1 and state[0] == ev
        assert math.isclose(float(ev - target), float(ev0 - target) * 0.7 ** k, rel_tol=1e-4), k
    # saturating frame count
    _, frame, new = D.exposure(dim, (F32(0), 0xFFFFFFFF, F32(0)))
    assert frame == 0xFFFFFFFF and new[1] == 0xFFFFFFFF


def test_fixed_mode_and_clamps():
    hist = D.histogram(gray(4, 4, 1e-4))[0]
    assert D.exposure(hist, exposure_mode=D.FIXED, exposure_ev=-2.0)[0] == F32(-2.0)
    assert D.exposure(hist, ev_max=3.0)[0] == F32(3.0)
    assert D.exposure(hist, ev_max=3.0, exposure_ev=0.5)[0] == F32(3.5)


def test_aces_zero_and_monotone():
    x = np.linspace(0, 100, 20001, dtype=F32)[:, None].repeat(3, axis=1)
    y = D.tone(x, D.ACES, 4.0)[:, 0]
    assert y[0] == 0 and y[-1] > 1.0
    assert (np.diff(y) >= -2.5e-7).all()  # monotone up to f32 rounding near the asymptote 2.51 / 2.43
    assert (np.diff(y[:2000]) > 0).all()


def test_reinhard_maps_white_to_one():
    for w in (1.0, 4.0, 11.2):
        x = np.array([[w, w, w]], F32)
        y = D.tone(x, D.REINHARD, w)
        assert np.allclose(y, 1.0, rtol=2e-6), (w, y)
        assert (D.tone(x * F32(0.5), D.REINHARD, w) < 1).all()
    # not metered-like luminances pass through to the clamp
    odd = np.array([[0.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [np.inf, 1.0, 1.0], [np.nan, 1.0, 1.0]], F32)
    assert np.array_equal(D.tone(odd, D.REINHARD, 4.0), odd, equal_nan=True)


def test_hable_maps_white_to_one():
    for w in (2.0, 4.0, 11.2):
        assert abs(float(D.tone(np.array([w], F32), D.HABLE, w)[0]) - 1.0) < 1e-6


def test_srgb_breakpoint(O):
    v = np.array([0.0031308, np.nextafter(F32(0.0031308), F32(1)), 0.0, 1.0], F32)
    t = D.transfer(O, v, D.SRGB, 2.2)
    assert t[0] == F32(12.92) * F32(0.0031308) and t[2] == 0
    assert abs(float(t[1]) - float(t[0])) < 1e-5  # continuous at the breakpoint
    assert abs(float(t[3]) - 1.0) < 1e-6


def test_round_against_reference(O):
    k = np.arange(256, dtype=F32)
    t = k / F32(255)
    assert np.array_equal(D.sat(t * F32(255) + F32(0.5)), k.astype(np.uint8))  # ROUND hits every code at k/255
    ref = D.sat(t * F32(255.999))
    assert np.array_equal(ref, np.floor(t * F32(255.999)).astype(np.uint8)) and (ref <= k).all()
    half = np.array([0.5], F32)
    assert D.sat(half * F32(255) + F32(0.5))[0] == 128 and D.sat(half * F32(255.999))[0] == 127  # rounds where truncation does not
    assert list(D.sat(np.array([np.nan, -1, 0, 254.99, 255, 1e9], F32))) == [0, 0, 0, 254, 255, 255]


def test_philox_port_matches_the_oracle(O):
    rng = np.random.default_rng(5)
    for _ in range(20):
        ctr = [int(v) for v in rng.integers(0, 2 ** 32, 4)]
        key = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        got = [int(w[()]) for w in D.philox(*ctr, *key)]
        assert got == O.philox(ctr, key)


def test_dither_mean_and_pattern(O):
    h, w = 64, 64
    for v in (0.2037, 0.5031, 0.9):
        img = gray(h, w, v)
        out = D.map_pixels(O, img, 0.0, 3, exposure_mode=D.FIXED, tonemap=D.CLAMP, transfer=D.LINEAR, quantiser=D.DITHER,
                           pixel_format=D.RGB8, seed=7)
        mean = out.astype(np.float64).mean()
        assert abs(mean - v * 255) < 0.5, (v, mean)
        assert len(np.unique(out)) == 2  # dithered between the two neighbouring codes
        other = D.map_pixels(O, img, 0.0, 4, exposure_mode=D.FIXED, tonemap=D.CLAMP, transfer=D.LINEAR,
                             quantiser=D.DITHER, pixel_format=D.RGB8, seed=7)
        assert not np.array_equal(out, other)  # the pattern changes with the frame
        again = D.map_pixels(O, img, 0.0, 3, exposure_mode=D.FIXED, tonemap=D.CLAMP, transfer=D.LINEAR,
                             quantiser=D.DITHER, pixel_format=D.RGB8, seed=7)
        assert np.array_equal(out, again)


def test_pixel_formats(O):
    img = np.random.default_rng(1).uniform(0, 2, (5, 7, 3)).astype(F32)
    kw = dict(exposure_mode=D.FIXED, tonemap=D.ACES, transfer=D.SRGB, quantiser=D.ROUND)
    rgb = D.map_pixels(O, img, 0.0, 0, pixel_format=D.RGB8, **kw)
    rgba = D.map_pixels(O, img, 0.0, 0, pixel_format=D.RGBA8, **kw)
    bgra = D.map_pixels(O, img, 0.0, 0, pixel_format=D.BGRA8, **kw)
    assert rgb.shape == (5, 7, 3) and rgba.shape == (5, 7, 4)
    assert np.array_equal(rgba[..., :3], rgb) and np.array_equal(bgra[..., :3], rgb[..., ::-1]) and (rgba[..., 3] == 255).all()


def test_identity_with_the_reference_conversion(O):
    rng = np.random.default_rng(2)
    img = rng.normal(0, 2, (9, 13, 3)).astype(F32)
    img.ravel()[:6] = [np.nan, np.inf, -1e30, -0.0, 0.0, 1e-40]
    kw = dict(exposure_mode=D.FIXED, tonemap=D.CLAMP, transfer=D.GAMMA, quantiser=D.REFERENCE, pixel_format=D.RGB8)
    for g in (2.2, 1.0, 1 / 3, 1.8):
        assert np.array_equal(D.map_pixels(O, img, 0.0, 0, gamma=g, **kw), O.output_rgb8(img, g)), g
    # the exceptions the header states: the reference's powf gives a negative value a positive power when 1/gamma is an even
    # integer, and turns -inf into +inf (255) unless 1/gamma is an odd integer; the clamp maps both to 0
    neg = img < 0
    assert neg.any()
    even = D.map_pixels(O, img, 0.0, 0, gamma=0.5, **kw)
    assert np.array_equal(even[~neg], O.output_rgb8(img, 0.5)[~neg]) and (even[neg] == 0).all()
    neg_inf = np.full((1, 1, 3), -np.inf, F32)
    assert (D.map_pixels(O, neg_inf, 0.0, 0, gamma=2.2, **kw) == 0).all() and (O.output_rgb8(neg_inf, 2.2) == 255).all()
    assert (D.map_pixels(O, neg_inf, 0.0, 0, gamma=1.0, **kw) == O.output_rgb8(neg_inf, 1.0)).all()


def test_overshadowed_auto_exposure_lands_near_the_key(golden_dir):
    img = np.load(os.path.join(golden_dir, "overshadowed_64x36_s16_mis.npy"))
    hist, metered = D.histogram(img)
    ev, _, _ = D.exposure(hist)
    y = D.lum32(img)[metered].astype(np.float64) * 2.0 ** float(ev)
    assert abs(math.log2(np.median(y)) - float(D.DEFAULTS["key_ev"])) <= 1.5, (ev, np.median(y))
    assert ev > 4  # a dark frame is pushed up by several stops


# ---- the library without a device ----
def test_display_symbols_and_structs(hb):
    lib = hb.lib()
    for sym in ("rt_display_opts_default", "rt_display_workspace_bytes", "rt_display_output_bytes", "rt_display_device",
                "rt_display", "rt_display_reset"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(abi.DisplayOpts) == abi.EXPECTED_SIZES["rt_display_opts"][1] == 104
    assert C.sizeof(abi.DisplayState) == abi.EXPECTED_SIZES["rt_display_state"][1] == 16


def test_display_opts_default(hb):
    o = abi.DisplayOpts()
    o.width, o.reserved[2], o.seed = 5, 9, 3
    assert hb.lib().rt_display_opts_default(C.byref(o)) == abi.RT_OK
    assert (o.width, o.height, o.seed) == (0, 0, 0) and list(o.reserved) == [0] * 8
    assert (o.exposure_mode, o.tonemap, o.transfer, o.quantiser, o.pixel_format) == (
        abi.RT_EXPOSURE_AUTO, abi.RT_TONEMAP_ACES, abi.RT_TRANSFER_SRGB, abi.RT_QUANT_DITHER, abi.RT_PIXEL_RGBA8)
    assert o.exposure_ev == 0 and o.key_ev == D.DEFAULTS["key_ev"] == F32(math.log2(0.18))
    assert (o.meter_low, o.meter_high) == (F32(0.1), F32(0.9)) and (o.ev_min, o.ev_max) == (-16, 16)
    assert (o.adaptation, o.white, o.gamma) == (1.0, 4.0, F32(2.2))
    assert hb.lib().rt_display_opts_default(None) == abi.RT_ERR_INVALID_ARGUMENT
    for k, v in D.DEFAULTS.items():
        assert F32(getattr(o, k)) == F32(v), k
    p = hb.display_opts(3, 4, tonemap="hable", pixel_format=abi.RT_PIXEL_RGB8, exposure_ev=1.5)
    assert (p.width, p.height, p.tonemap, p.pixel_format, p.exposure_ev) == (3, 4, abi.RT_TONEMAP_HABLE, abi.RT_PIXEL_RGB8, 1.5)
    with pytest.raises(ValueError):
        hb.display_opts(3, 4, tone="aces")
    with pytest.raises(ValueError):
        hb.display_opts(3, 4, tonemap="agx")


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (33, 17), (64, 32), (1920, 1080), (3840, 2160), (1 << 16, 1 << 15)])
def test_workspace_and_output_bytes(hb, w, h):
    n = w * h
    o = hb.display_opts(w, h)
    assert hb.display_workspace_bytes(o) == 16 + 1024 * min(256, max(1, -(-n // 2048)))
    assert hb.display_output_bytes(o) == 4 * n
    o.pixel_format = abi.RT_PIXEL_BGRA8
    assert hb.display_output_bytes(o) == 4 * n
    o.pixel_format = abi.RT_PIXEL_RGB8
    assert hb.display_output_bytes(o) == 3 * n


def test_bytes_reject(hb):
    lib = hb.lib()
    n = C.c_uint64()
    for fn in (lib.rt_display_workspace_bytes, lib.rt_display_output_bytes):
        for w, h in ((0, 5), (5, 0)):
            assert fn(C.byref(hb.display_opts(w, h)), C.byref(n)) == abi.RT_ERR_INVALID_ARGUMENT
        assert fn(C.byref(hb.display_opts(1 << 16, (1 << 15) + 1)), C.byref(n)) == abi.RT_ERR_UNSUPPORTED
        assert fn(None, C.byref(n)) == abi.RT_ERR_INVALID_ARGUMENT
        assert fn(C.byref(hb.display_opts(2, 2)), None) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_display_output_bytes(C.byref(hb.display_opts(2, 2, pixel_format=3)), C.byref(n)) == abi.RT_ERR_INVALID_ARGUMENT


def _expect(lib, rc, code, words):
    assert rc == code, (rc, code, lib.rt_last_error())
    msg = lib.rt_last_error().decode()
    assert all(word in msg for word in words), msg


def _aligned(nbytes):
    keep = np.zeros(nbytes // 4 + 8, np.float32)
    return keep, (keep.ctypes.data + 15) // 16 * 16


def test_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    h, w = 9, 16
    n = h * w
    img = np.zeros((h, w, 3), np.float32)
    k1, ws = _aligned(hb.display_workspace_bytes(hb.display_opts(w, h)))
    k2, out = _aligned(4 * n)
    k3, state = _aligned(16)
    k4, hist = _aligned(1024)
    rgb = img.ctypes.data
    inv = abi.RT_ERR_INVALID_ARGUMENT

    def dev(opts, src=rgb, st=state, wsp=ws, o=out, hi=hist, scene=s._h):
        return lib.rt_display_device(scene, C.c_void_p(src), C.byref(opts) if opts is not None else None, C.c_void_p(st),
                                     C.c_void_p(wsp), C.c_void_p(o), C.c_void_p(hi), C.c_void_p(0))

    def host(opts, src=rgb, st=state, wsp=None, o=out, hi=hist, scene=s._h):
        return lib.rt_display(scene, C.c_void_p(src), C.byref(opts) if opts is not None else None, C.c_void_p(o),
                              C.c_void_p(st), C.c_void_p(hi))

    good = hb.display_opts(w, h)
    for call in (dev, host):
        _expect(lib, call(good), abi.RT_ERR_NO_DEVICE, ["host-only"])
        _expect(lib, call(good, st=None, hi=None), abi.RT_ERR_NO_DEVICE, ["host-only"])
        for kw in (dict(src=None), dict(o=None), dict(scene=None)):
            _expect(lib, call(good, **kw), inv, ["null"])
        _expect(lib, call(None), inv, ["null"])
        for ww, hh in ((0, h), (w, 0)):
            _expect(lib, call(hb.display_opts(ww, hh)), inv, ["width"])
        for k in ("exposure_mode", "tonemap", "transfer", "quantiser", "pixel_format"):
            for bad in (-1, 4 if k == "tonemap" else (2 if k == "exposure_mode" else 3)):
                _expect(lib, call(hb.display_opts(w, h, **{k: bad})), inv, [k])
        bad_opts = [dict(exposure_ev=float("nan")), dict(exposure_ev=float("inf")), dict(key_ev=float("-inf")),
                    dict(meter_low=-0.1), dict(meter_low=0.5, meter_high=0.5), dict(meter_high=1.01),
                    dict(meter_low=float("nan")), dict(ev_min=2.0, ev_max=1.0), dict(ev_min=float("-inf")),
                    dict(ev_max=float("nan")), dict(adaptation=0.0), dict(adaptation=1.5), dict(adaptation=float("nan")),
                    dict(white=0.0), dict(white=-1.0), dict(white=float("inf")), dict(gamma=0.0), dict(gamma=float("nan"))]
        for kw in bad_opts:
            assert call(hb.display_opts(w, h, **kw)) == inv, kw
        for edge in (dict(meter_low=0.0, meter_high=1.0), dict(ev_min=3.0, ev_max=3.0), dict(adaptation=1e-6),
                     dict(exposure_mode="fixed", tonemap="hable", transfer="linear", quantiser="reference", pixel_format="bgra8")):
            _expect(lib, call(hb.display_opts(w, h, **edge)), abi.RT_ERR_NO_DEVICE, ["host-only"])
        _expect(lib, call(hb.display_opts(1 << 16, (1 << 15) + 1)), abi.RT_ERR_UNSUPPORTED, ["2^31"])
        # buffers written against every other buffer
        _expect(lib, call(good, o=rgb), inv, ["overlaps"])
        _expect(lib, call(good, o=rgb + 12 * n - 4), inv, ["overlaps"])
        _expect(lib, call(good, st=rgb + 8), inv, ["overlaps"])
        _expect(lib, call(good, hi=rgb + 4), inv, ["overlaps"])
        _expect(lib, call(good, hi=out + 16), inv, ["overlaps"])
        _expect(lib, call(good, st=hist + 1008), inv, ["overlaps"])
        _expect(lib, call(good, st=out), inv, ["overlaps"])
        # RGB8 output is 3 bytes per pixel: a state right after it is fine
        rgb8 = hb.display_opts(w, h, pixel_format="rgb8")
        _expect(lib, call(rgb8, st=out + 3 * n), abi.RT_ERR_NO_DEVICE, ["host-only"])
        _expect(lib, call(good, st=out + 3 * n), inv, ["overlaps"])
    # the device call's workspace
    _expect(lib, dev(good, wsp=None), inv, ["workspace"])
    _expect(lib, dev(good, wsp=ws + 4), inv, ["aligned"])
    _expect(lib, dev(good, wsp=out), inv, ["overlaps"])
    _expect(lib, dev(good, st=ws + 16), inv, ["overlaps"])
    _expect(lib, dev(good, wsp=(rgb + 15) // 16 * 16), inv, ["overlaps"])
    # the host call takes no workspace: nothing to check there
    # reset needs no device
    assert lib.rt_display_reset(s._h) == abi.RT_OK
    assert lib.rt_display_reset(None) == inv
    s.display_reset()
    assert bytes(s.display_state()) == bytes(16)
    with pytest.raises(hb.RtHipError) as e:
        s.display(img)
    assert e.value.code == abi.RT_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        s.display(img[..., :2])


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() {\n'
           'rt_hip::DisplayOptions d; d.tonemap = RT_TONEMAP_HABLE; d.pixel_format = RT_PIXEL_RGB8; d.adaptation = 0.3f;\n'
           'rt_display_opts (*f)(const rt_hip::DisplayOptions &, uint32_t, uint32_t) = &rt_hip::display_opts;\n'
           'std::vector<uint8_t> (rt_hip::Display::*g)(const std::vector<float> &, rt_display_state *, std::vector<uint32_t> *)'
           ' = &rt_hip::Display::operator();\n'
           'void (rt_hip::Display::*r)() = &rt_hip::Display::reset;\n'
           '(void)f; (void)g; (void)r; (void)d; return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)
