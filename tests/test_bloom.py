"""The bloom stage (rt_bloom, include/rt_hip.h) without a GPU: the ABI surface, the workspace formula and every status code on a
host-only scene, then the numpy checker (tests/bloom_checker.py) held to hand-computed cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bloom_checker as B
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32
INVALID, UNSUPPORTED, NO_DEVICE = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE


# ---- the C-ABI boundary ----
def test_struct_size_against_a_compiled_sizeof(hb, tmp_path):
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){'
           'printf("%zu %u\\n", sizeof(rt_bloom_opts), RT_ABI_VERSION); return 0;}')
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    size, version = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == C.sizeof(abi.BloomOpts) == abi.EXPECTED_SIZES["rt_bloom_opts"][1] == 64
    assert abi.EXPECTED_SIZES["rt_bloom_opts"][0] is abi.BloomOpts and int(version) == abi.RT_ABI_VERSION == 2
    lib = hb.lib()
    for sym in ("rt_bloom_opts_default", "rt_bloom_workspace_bytes", "rt_bloom_device", "rt_bloom"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert sum("bloom" in name for name in abi.EXPORTED_SYMBOLS) == 4


def test_defaults(hb):
    lib = hb.lib()
    o = abi.BloomOpts()
    o.width, o.levels, o.knee = 5, 99, 7.0
    o.reserved[5] = 9
    assert lib.rt_bloom_opts_default(C.byref(o)) == abi.RT_OK
    assert (o.width, o.height) == (0, 0) and list(o.reserved) == [0] * 6
    assert (o.threshold, o.knee, o.intensity, o.scatter) == (1.0, 0.5, F32(0.05), F32(0.7))
    assert (o.levels, o.exposure_ev, o.clamp_max, o.fuse_tail) == (6, 0.0, 65504.0, 1)
    for k, v in B.DEFAULTS.items():
        assert F32(getattr(o, k)) == F32(v), k
    assert set(abi.BLOOM_OPTIONS) == set(B.DEFAULTS) and abi.BLOOM_MAX_LEVELS == B.MAX_LEVELS
    assert lib.rt_bloom_opts_default(None) == INVALID
    p = hb.bloom_opts(3, 4, levels=2, knee=0.25)
    assert (p.width, p.height, p.levels, p.knee, p.scatter) == (3, 4, 2, 0.25, F32(0.7))
    with pytest.raises(ValueError):
        hb.bloom_opts(3, 4, radius=2)


@pytest.mark.parametrize("w,h", [(1, 1), (13, 11), (150, 130), (1920, 1080)])
@pytest.mark.parametrize("levels", [1, 6, 12])
def test_workspace_bytes(hb, w, h, levels):
    """sum over the n levels of 16*ceil(12*w_i*h_i / 16), written out here independently of the checker"""
    total, a, b, n = 0, w, h, 0
    while n < levels:
        a, b, n = -(-a // 2), -(-b // 2), n + 1
        total += -(-12 * a * b // 16) * 16
        if a == 1 and b == 1:
            break
    assert hb.bloom_workspace_bytes(hb.bloom_opts(w, h, levels=levels)) == total == B.workspace_bytes(w, h, levels)
    assert total % 16 == 0 and total >= 16


def test_level_sizes_and_tail():
    assert B.level_sizes(150, 130, 6) == [(75, 65), (38, 33), (19, 17), (10, 9), (5, 5), (3, 3)]
    assert B.level_sizes(1920, 1080, 6) == [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]
    assert B.level_sizes(13, 11, 12) == [(7, 6), (4, 3), (2, 2), (1, 1)] and B.level_sizes(1, 1, 12) == [(1, 1)]
    assert B.level_sizes(2, 1, 12) == [(1, 1)] and len(B.level_sizes(1920, 1080, 12)) == 11
    assert B.workspace_bytes(1, 1, 1) == 16 and B.workspace_bytes(13, 11, 12) == 512 + 144 + 48 + 16  # 12 * 42 = 504 rounds up
    # the fused tail: levels t .. n-1 hold at most 4096 pixels together, t >= 1
    assert B.tail_from(150, 130, 6) == 1 and B.tail_from(1920, 1080, 6) == 4 and B.tail_from(300, 200, 6) == 2
    assert B.tail_from(13, 11, 1) == 1 and B.tail_from(1, 1, 6) == 1 and B.tail_from(13, 11, 6) == 1


def _expect(lib, rc, code, words=()):
    assert rc == code, (rc, code, lib.rt_last_error())
    msg = lib.rt_last_error().decode()
    assert all(word in msg for word in words), msg


def _aligned(nbytes):
    keep = np.zeros(nbytes // 4 + 8, np.float32)
    return keep, (keep.ctypes.data + 15) // 16 * 16


def test_workspace_bytes_rejects(hb):
    lib = hb.lib()
    n = C.c_uint64()
    fn = lib.rt_bloom_workspace_bytes
    for w, h in ((0, 5), (5, 0)):
        _expect(lib, fn(C.byref(hb.bloom_opts(w, h)), C.byref(n)), INVALID, ["width"])
    for levels in (0, 13):
        _expect(lib, fn(C.byref(hb.bloom_opts(4, 4, levels=levels)), C.byref(n)), INVALID, ["levels"])
    _expect(lib, fn(C.byref(hb.bloom_opts(1 << 16, (1 << 15) + 1)), C.byref(n)), UNSUPPORTED, ["2^31"])
    _expect(lib, fn(None, C.byref(n)), INVALID, ["null"])
    _expect(lib, fn(C.byref(hb.bloom_opts(2, 2)), None), INVALID, ["null"])


def test_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    h, w = 9, 16
    n = h * w
    good = hb.bloom_opts(w, h)
    ws_bytes = hb.bloom_workspace_bytes(good)
    k0, rgb = _aligned(12 * n)
    k1, ws = _aligned(ws_bytes)
    k2, out = _aligned(12 * n)
    k3, state = _aligned(16)

    def dev(opts, src=rgb, st=state, wsp=ws, o=out, scene=s._h):
        return lib.rt_bloom_device(scene, C.c_void_p(src), C.byref(opts) if opts is not None else None, C.c_void_p(st),
                                   C.c_void_p(wsp), C.c_void_p(o), C.c_void_p(0))

    def host(opts, src=rgb, st=state, wsp=None, o=out, scene=s._h):
        return lib.rt_bloom(scene, C.c_void_p(src), C.byref(opts) if opts is not None else None, C.c_void_p(st), C.c_void_p(o))

    for call in (dev, host):
        _expect(lib, call(good), NO_DEVICE, ["host-only"])
        _expect(lib, call(good, st=None), NO_DEVICE, ["host-only"])
        for kw in (dict(src=None), dict(o=None), dict(scene=None)):
            _expect(lib, call(good, **kw), INVALID, ["null"])
        _expect(lib, call(None), INVALID, ["null"])
        for ww, hh in ((0, h), (w, 0)):
            _expect(lib, call(hb.bloom_opts(ww, hh)), INVALID, ["width"])
        bad = [dict(threshold=-0.5), dict(threshold=float("nan")), dict(threshold=float("inf")),
               dict(knee=-0.1), dict(knee=1.5), dict(knee=float("nan")),
               dict(intensity=-1.0), dict(intensity=float("inf")), dict(intensity=float("nan")),
               dict(scatter=-0.1), dict(scatter=1.01), dict(scatter=float("nan")),
               dict(levels=0), dict(levels=13),
               dict(exposure_ev=float("nan")), dict(exposure_ev=float("-inf")),
               dict(clamp_max=0.0), dict(clamp_max=-1.0), dict(clamp_max=float("inf")), dict(clamp_max=float("nan")),
               dict(fuse_tail=2)]
        for kw in bad:
            _expect(lib, call(hb.bloom_opts(w, h, **kw)), INVALID, [next(iter(kw))])
        r = hb.bloom_opts(w, h)
        r.reserved[3] = 1
        _expect(lib, call(r), INVALID, ["reserved"])
        for edge in (dict(threshold=0.0), dict(knee=0.0), dict(knee=1.0), dict(intensity=0.0), dict(scatter=0.0), dict(scatter=1.0),
                     dict(levels=1), dict(levels=12), dict(exposure_ev=-30.0), dict(clamp_max=1e-3), dict(fuse_tail=0)):
            _expect(lib, call(hb.bloom_opts(w, h, **edge)), NO_DEVICE, ["host-only"])
        _expect(lib, call(hb.bloom_opts(1 << 16, (1 << 15) + 1)), UNSUPPORTED, ["2^31"])
        # every pair of buffers, except out == rgb exactly
        _expect(lib, call(good, o=rgb), NO_DEVICE, ["host-only"])  # in place
        _expect(lib, call(good, o=rgb + 4), INVALID, ["overlap"])
        _expect(lib, call(good, o=rgb + 12 * n - 4), INVALID, ["overlap"])
        _expect(lib, call(good, o=rgb - 12 * n + 4), INVALID, ["overlap"])
        _expect(lib, call(good, st=rgb + 8), INVALID, ["overlap"])
        _expect(lib, call(good, st=out + 12 * n - 4), INVALID, ["overlap"])
        _expect(lib, call(good, st=out + 12 * n), NO_DEVICE, ["host-only"])  # right behind the output: disjoint
    # the device call's workspace
    _expect(lib, dev(good, wsp=None), INVALID, ["workspace"])
    _expect(lib, dev(good, wsp=ws + 4), INVALID, ["aligned"])
    _expect(lib, dev(good, wsp=out), INVALID, ["overlap"])
    _expect(lib, dev(good, wsp=rgb), INVALID, ["overlap"])
    _expect(lib, dev(good, st=ws + ws_bytes - 16), INVALID, ["overlap"])
    _expect(lib, dev(good, o=rgb, wsp=rgb), INVALID, ["overlap"])
    # the Python wrappers
    img = np.zeros((h, w, 3), F32)
    with pytest.raises(hb.RtHipError) as e:
        s.bloom(img)
    assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        s.bloom(img[..., :2])


# ---- the checker on hand-computed cases ----
def test_below_threshold_with_no_knee_returns_the_input(O):
    rng = np.random.default_rng(1)
    img = rng.uniform(0.0, 0.999, (9, 14, 3)).astype(F32)
    out = B.bloom(O, img, knee=0.0, intensity=1.0)
    assert out.tobytes() == img.tobytes()
    assert not B.bright(img, F32(1), knee=0.0).any()
    assert B.bright(img, F32(1), knee=0.5).any()  # the knee reaches below the threshold
    assert B.bloom(O, img, intensity=0.0).tobytes() == img.tobytes()


def test_a_pixel_at_the_threshold():
    """with no knee it contributes exactly 0; with a knee it contributes the header's soft = (k*k)/(4k + 1e-5)"""
    for th in (1.0, 0.25, 3.0):
        px = np.full((1, 1, 3), th, F32)
        assert F32(B.lum32(px)[0, 0]) == F32(th)  # grey: Y is the value itself
        assert not B.bright(px, F32(1), threshold=th, knee=0.0).any()
        k = F32(th) * F32(0.5)
        soft = (k * k) / (F32(4) * k + F32(1e-5))
        assert (B.bright(px, F32(1), threshold=th, knee=0.5) == F32(th) * (soft / F32(th))).all() and soft > 0
        above = B.bright(px * F32(3), F32(1), threshold=th, knee=0.0)  # far above: Y - threshold of Y
        y = F32(B.lum32(px * F32(3))[0, 0])
        assert (above == (px * F32(3)) * ((y - F32(th)) / y)).all()


def test_single_bright_pixel_is_symmetric_and_non_negative(O):
    """A 16 x 16 frame has no middle pixel: the over-range patch is the 2 x 2 block about the centre (one pixel of level 0).  The
    taps mirror exactly, but a mirrored sum adds its terms in the opposite order, so the symmetry holds to rounding, not to the
    bit: at most ~50 non-negative terms per output value, 2^-24 each and no cancellation -- 2e-5 relative is generous."""
    img = np.zeros((16, 16, 3), F32)
    img[7:9, 7:9] = (40.0, 20.0, 10.0)
    resp = B.bloom(O, img, intensity=1.0)
    assert np.isfinite(resp).all() and (resp >= 0).all() and (resp >= img).all() and (resp[0, 0] > 0).all()
    assert np.allclose(resp, resp[:, ::-1], rtol=2e-5, atol=0) and np.allclose(resp, resp[::-1], rtol=2e-5, atol=0)
    assert np.allclose(resp, resp.transpose(1, 0, 2), rtol=2e-5, atol=0)
    one = B.bloom(O, img, intensity=1.0, levels=1) - img  # one level: level 0 pixels 3 and 4 hold it, fine pixels 5 .. 10 see them
    assert (one >= 0).all() and one[7, 7, 0] > one[7, 5, 0] > 0 and one[7, 4, 0] == 0
    single = np.zeros((16, 16, 3), F32)
    single[8, 8] = (40.0, 20.0, 10.0)
    assert (B.bloom(O, single, intensity=1.0) >= single).all()


def test_non_finite_and_negative_pixels_pass_through_and_never_spread(O):
    rng = np.random.default_rng(2)
    img = (rng.uniform(0.0, 1.0, (11, 13, 3)) * np.exp2(rng.uniform(-2, 5, (11, 13, 1)))).astype(F32)
    odd = {(2, 3, 0): np.nan, (5, 6, 1): np.inf, (7, 1, 2): -np.inf, (9, 10, 0): -4.0, (0, 0, 1): -1e30}
    dirty, zeroed = img.copy(), img.copy()
    for at, v in odd.items():
        dirty[at], zeroed[at] = v, 0.0
    out, ref = B.bloom(O, dirty, intensity=0.5), B.bloom(O, zeroed, intensity=0.5)
    for at, v in odd.items():  # c + the bloom its neighbours cast on it (ref there: 0 + that term): NaN, inf and -1e30 stay what they are
        want = F32(v) + ref[at]
        assert (np.isnan(out[at]) and np.isnan(v)) or out[at] == want, at
        assert np.isfinite(v) or np.isnan(v) or out[at] == F32(v)
    assert out[0, 0, 1] == F32(-1e30) and out[9, 10, 0] < 0
    mask = np.ones(img.shape, bool)
    for at in odd:
        mask[at] = False
    assert np.isfinite(out[mask]).all() and out[mask].tobytes() == ref[mask].tobytes()
    assert (out[mask] > dirty[mask]).all()  # and the blur did reach them
    assert np.isfinite(B.bright(dirty, F32(1))).all() and (B.bright(dirty, F32(1)) >= 0).all()


def test_clamp_max_bounds_a_firefly(O):
    hue = np.array([0.5, 1.0, 0.25], F32)
    cm = F32(100.0)
    fly, capped = np.zeros((9, 9, 3), F32), np.zeros((9, 9, 3), F32)
    fly[4, 4] = hue * F32(1e30)
    y = F32(B.lum32(fly[4, 4]))
    capped[4, 4] = fly[4, 4] * (cm / y)  # luminance clamp_max, the same hue (the header's own scaling)
    b_fly, b_cap = B.bright(fly, F32(1), clamp_max=cm), B.bright(capped, F32(1), clamp_max=cm)
    assert np.isfinite(b_fly).all() and abs(float(B.lum32(b_fly[4, 4])) - 99.0) < 1e-3  # Y - threshold of a pixel of Y = 100
    assert np.allclose(b_fly, b_cap, rtol=1e-6, atol=0)
    r_fly = B.bloom(O, fly, clamp_max=cm, intensity=1.0) - fly
    r_cap = B.bloom(O, capped, clamp_max=cm, intensity=1.0) - capped
    far = np.ones((9, 9), bool)
    far[4, 4] = False  # (at the pixel itself 1e30 + bloom is 1e30)
    assert np.allclose(r_fly[far], r_cap[far], rtol=1e-5, atol=0) and r_fly[far].max() < 100.0


def _r4(a, b, c, d):
    return ((a * F32(0.125) + b * F32(0.375)) + c * F32(0.375)) + d * F32(0.125)


def _even(lo, hi):
    return lo * F32(0.25) + hi * F32(0.75)


def _odd(lo, hi):
    return lo * F32(0.75) + hi * F32(0.25)


def test_1x1_and_2x1_by_hand(O):
    """every clamped tap of a 1 x 1 image is the pixel itself; the sums are still rounded one by one, as written here"""
    v = np.array([6.0, 3.0, 2.0], F32)
    y = F32(F32(0.2126) * F32(6) + F32(0.7152) * F32(3)) + F32(0.0722) * F32(2)
    b = v * ((y - F32(1)) / y)  # far above the knee: wgt = (Y - threshold) / Y
    assert B.bright(v[None, None], F32(1)).tobytes() == b.tobytes()
    t = _r4(b, b, b, b)
    b0 = _r4(t, t, t, t)  # level 0, 1 x 1: n = 1 and U_0 = B_0
    assert B.reduce(b[None, None]).tobytes() == b0.tobytes()
    h = _even(b0, b0)
    e = _even(h, h)
    assert B.expand(b0[None, None], 1, 1).tobytes() == e.tobytes() and np.allclose(e, b, rtol=1e-6)
    out = B.bloom(O, v[None, None], intensity=0.5)
    assert out.shape == (1, 1, 3) and out.tobytes() == (v + (F32(0.5) * e) / F32(1)).tobytes()
    # 2 x 1: level 0 is 1 x 1 with the taps l l r r; pixel 0 is even, pixel 1 odd
    lr = np.array([[[6.0, 3.0, 2.0], [0.0, 1.0, 0.0]]], F32)
    br = B.bright(lr, F32(1))
    assert br[0, 0].tobytes() == b.tobytes() and (br[0, 1] > 0).any()  # Y = 0.7152 lies inside the knee
    t = _r4(br[0, 0], br[0, 0], br[0, 1], br[0, 1])
    b0 = _r4(t, t, t, t)
    h0, h1 = _even(b0, b0), _odd(b0, b0)
    e = np.stack([_even(h0, h0), _even(h1, h1)])[None]
    out = B.bloom(O, lr, intensity=0.25)
    assert out.tobytes() == (lr + (F32(0.25) * e) / F32(1)).tobytes()
    # +1 EV doubles the frame ahead of the threshold and divides the bloom by 2 behind it
    assert B.scale(O, 1.0) == F32(2) and B.scale(O, 0.0) == F32(1) and B.scale(O, -3.0) == F32(0.125)
    x = v * F32(2)
    y2 = F32(F32(0.2126) * x[0] + F32(0.7152) * x[1]) + F32(0.0722) * x[2]
    b = x * ((y2 - F32(1)) / y2)
    t = _r4(b, b, b, b)
    b0 = _r4(t, t, t, t)
    h = _even(b0, b0)
    up = B.bloom(O, v[None, None], intensity=0.5, exposure_ev=1.0)
    assert up.tobytes() == (v + (F32(0.5) * _even(h, h)) / F32(2)).tobytes()
    assert B.bloom(O, v[None, None], intensity=0.5, exposure_ev=0.25, ev=1.0).tobytes() == up.tobytes()  # ev overrides


def test_levels_beyond_1x1(O):
    rng = np.random.default_rng(3)
    img = (rng.uniform(0, 1, (11, 13, 3)) * 8).astype(F32)
    assert len(B.level_sizes(13, 11, 12)) == 4
    at = B.bloom(O, img, levels=4)
    for levels in (5, 6, 12):
        assert B.bloom(O, img, levels=levels).tobytes() == at.tobytes()
    assert B.bloom(O, img, levels=3).tobytes() != at.tobytes()


def test_scatter_and_reduce_expand_shapes():
    rng = np.random.default_rng(4)
    b = rng.uniform(0, 4, (7, 10, 3)).astype(F32)
    r = B.reduce(b)
    assert r.shape == (4, 5, 3) and B.expand(r, 10, 7).shape == (7, 10, 3) and B.expand(r, 9, 8).shape == (8, 9, 3)
    flat = np.full((6, 9, 3), 2.5, F32)
    assert (B.reduce(flat) == F32(2.5)).all() and (B.expand(B.reduce(flat), 9, 6) == F32(2.5)).all()  # the weights sum to 1 exactly
    assert B.pyramid(b, 6, 0.0).tobytes() == r.tobytes()  # scatter 0: U_0 is B_0
    # interior taps by hand
    assert r[1, 2, 0] == B._reduce_axis(B._reduce_axis(b, 1), 0)[1, 2, 0]
    t = [((b[y, 3, 0] * F32(0.125) + b[y, 4, 0] * F32(0.375)) + b[y, 5, 0] * F32(0.375)) + b[y, 6, 0] * F32(0.125) for y in (1, 2, 3, 4)]
    assert r[1, 2, 0] == ((t[0] * F32(0.125) + t[1] * F32(0.375)) + t[2] * F32(0.375)) + t[3] * F32(0.125)
    e = B.expand(r, 10, 7)
    hx = lambda y, a, wa, c, wc: r[y, a, 1] * F32(wa) + r[y, c, 1] * F32(wc)  # noqa: E731
    assert e[2, 4, 1] == hx(0, 1, 0.25, 2, 0.75) * F32(0.25) + hx(1, 1, 0.25, 2, 0.75) * F32(0.75)  # even, even
    assert e[3, 5, 1] == hx(1, 2, 0.75, 3, 0.25) * F32(0.75) + hx(2, 2, 0.75, 3, 0.25) * F32(0.25)  # odd, odd
    assert e[0, 9, 1] == hx(0, 4, 0.75, 4, 0.25) * F32(0.25) + hx(0, 4, 0.75, 4, 0.25) * F32(0.75)  # clamped at both borders
