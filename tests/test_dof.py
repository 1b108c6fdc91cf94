"""The depth-of-field stage (rt_dof, include/rt_hip.h) without a GPU: the ABI surface, the workspace formula, the options made from
a camera and every status code on a host-only scene, then the numpy checker (tests/dof_checker.py) held to hand-computed cases."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import dof_checker as K
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32
INF = F32(np.inf)
INVALID, UNSUPPORTED, NO_DEVICE = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE
SYMBOLS = ("rt_dof_opts_default", "rt_dof_opts_from_camera", "rt_dof_workspace_bytes", "rt_dof_device", "rt_dof", "rt_render_dof")
CAMERA_A = dict(origin=(13.0, 2.0, 3.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), fov=20.0, aspect_ratio=float(F32(16.0) / F32(9.0)),
                aperture=0.1, focus_dist=10.0)
CAMERA_B = dict(origin=(0.0, 1.2, 5.0), lookat=(0.5, 0.6, 0.0), vup=(0.1, 1.0, 0.0), fov=55.0, aspect_ratio=1.25, aperture=0.4,
                focus_dist=3.5)


# ---- the C-ABI boundary ----
def test_struct_size_against_a_compiled_sizeof(hb, tmp_path):
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){'
           'printf("%zu %u\\n", sizeof(rt_dof_opts), RT_ABI_VERSION); return 0;}')
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    size, version = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == C.sizeof(abi.DofOpts) == abi.EXPECTED_SIZES["rt_dof_opts"][1] == 64
    assert abi.EXPECTED_SIZES["rt_dof_opts"][0] is abi.DofOpts and int(version) == abi.RT_ABI_VERSION == 2
    lib = hb.lib()
    for sym in SYMBOLS:
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert sum("dof" in name for name in abi.EXPORTED_SYMBOLS) == len(SYMBOLS)


def test_defaults(hb):
    lib = hb.lib()
    o = abi.DofOpts()
    o.width, o.max_radius, o.blur_scale = 5, 99, 7.0
    o.reserved[9] = 9
    assert lib.rt_dof_opts_default(C.byref(o)) == abi.RT_OK
    assert (o.width, o.height) == (0, 0) and list(o.reserved) == [0] * 10
    assert (o.focus_distance, o.blur_scale, o.max_radius, o.planar_depth) == (10.0, 0.0, 8, 1)
    for k, v in K.DEFAULTS.items():
        assert F32(getattr(o, k)) == F32(v), k
    assert set(abi.DOF_OPTIONS) == set(K.DEFAULTS) and abi.DOF_MAX_RADIUS == K.MAX_RADIUS == 16
    assert lib.rt_dof_opts_default(None) == INVALID
    p = hb.dof_opts(3, 4, max_radius=2, blur_scale=0.25)
    assert (p.width, p.height, p.max_radius, p.blur_scale, p.focus_distance) == (3, 4, 2, 0.25, 10.0)
    with pytest.raises(ValueError):
        hb.dof_opts(3, 4, levels=2)


def _expect(lib, rc, code, words=()):
    assert rc == code, (rc, code, lib.rt_last_error())
    msg = lib.rt_last_error().decode()
    assert all(word in msg for word in words), msg


@pytest.mark.parametrize("w,h", [(1, 1), (13, 11), (67, 35), (1920, 1080)])
def test_workspace_bytes(hb, w, h):
    """(r, depthkey) per pixel, rounded up to 16 bytes"""
    total = -(-8 * w * h // 16) * 16
    assert hb.dof_workspace_bytes(hb.dof_opts(w, h)) == total == K.workspace_bytes(w, h)
    assert total % 16 == 0 and total >= 16


def test_workspace_bytes_rejects(hb):
    lib = hb.lib()
    n = C.c_uint64()
    fn = lib.rt_dof_workspace_bytes
    for w, h in ((0, 5), (5, 0)):
        _expect(lib, fn(C.byref(hb.dof_opts(w, h)), C.byref(n)), INVALID, ["width"])
    _expect(lib, fn(C.byref(hb.dof_opts(1 << 16, (1 << 15) + 1)), C.byref(n)), UNSUPPORTED, ["2^31"])
    _expect(lib, fn(None, C.byref(n)), INVALID, ["null"])
    _expect(lib, fn(C.byref(hb.dof_opts(2, 2)), None), INVALID, ["null"])


@pytest.mark.parametrize("params", [CAMERA_A, CAMERA_B], ids=["a", "b"])
def test_opts_from_camera_against_the_formula(hb, params):
    """blur_scale = ((aperture*0.5f) * (float)(W - 1)) / |horizontal| in f32, the rest as documented"""
    cam = hb.camera_new(**params)
    hz = np.array(cam.horizontal[:], F32)
    length = np.sqrt((hz[0] * hz[0] + hz[1] * hz[1]) + hz[2] * hz[2])
    for w, h in ((64, 36), (1920, 1080)):
        o = hb.dof_opts_from_camera(cam, params["aperture"], params["focus_dist"], w, h)
        want = ((F32(params["aperture"]) * F32(0.5)) * F32(w - 1)) / length
        assert F32(o.blur_scale) == want and want > 0
        assert (o.width, o.height, o.planar_depth, o.max_radius) == (w, h, 1, 8) and list(o.reserved) == [0] * 10
        assert F32(o.focus_distance) == F32(params["focus_dist"])
        # what the number means: the focus plane is |horizontal| wide (camera_new scales the axis by focus_dist), so a lens
        # of radius aperture / 2 seen on it covers that many pixels
        tan_half = math.tan(math.radians(params["fov"]) / 2)
        plane_width = 2 * tan_half * params["focus_dist"]  # the field of view is the horizontal one
        assert abs(float(want) - params["aperture"] / 2 * (w - 1) / plane_width) < 1e-4 * float(want)
    assert hb.dof_opts_from_camera(cam, 0.3, 4.0, 64, 36, max_radius=16).max_radius == 16
    assert hb.dof_opts_from_camera(cam, 0.0, 4.0, 64, 36).blur_scale == 0.0


def test_opts_from_camera_rejects(hb):
    lib = hb.lib()
    cam = hb.camera_new(**CAMERA_A)
    o = abi.DofOpts()

    def call(camera=cam, aperture=0.1, focus=10.0, w=64, h=36, out=o):
        return lib.rt_dof_opts_from_camera(C.byref(out) if out is not None else None, C.byref(camera) if camera is not None else None,
                                           C.c_float(aperture), C.c_float(focus), C.c_uint32(w), C.c_uint32(h))

    assert call() == abi.RT_OK
    _expect(lib, call(out=None), INVALID, ["null"])
    _expect(lib, call(camera=None), INVALID, ["null"])
    for v in (-0.1, float("nan"), float("inf")):
        _expect(lib, call(aperture=v), INVALID, ["aperture"])
    for v in (0.0, -1.0, float("nan"), float("inf")):
        _expect(lib, call(focus=v), INVALID, ["focus_dist"])
    _expect(lib, call(w=1), INVALID, ["width"])
    _expect(lib, call(h=1), INVALID, ["width"])
    flat = abi.Camera()
    _expect(lib, call(camera=flat), INVALID, ["horizontal"])


def _aligned(nbytes):
    keep = np.zeros(nbytes // 4 + 8, np.float32)
    return keep, (keep.ctypes.data + 15) // 16 * 16


def test_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    cam = hb.camera_new(**ls.camera_params)
    h, w = 9, 16
    n = h * w
    good = hb.dof_opts(w, h, blur_scale=3.0)
    ws_bytes = hb.dof_workspace_bytes(good)
    k0, rgb = _aligned(12 * n)
    k1, ws = _aligned(ws_bytes)
    k2, out = _aligned(12 * n)
    k3, depth = _aligned(4 * n)
    k4, coc = _aligned(4 * n)

    def ptr(v):
        return C.c_void_p(v)

    def dev(opts, src=rgb, z=depth, camera=cam, wsp=ws, o=out, c=coc, scene=s._h):
        return lib.rt_dof_device(scene, ptr(src), ptr(z), C.byref(camera) if camera is not None else None,
                                 C.byref(opts) if opts is not None else None, ptr(wsp), ptr(o), ptr(c), ptr(0))

    def host(opts, src=rgb, z=depth, camera=cam, wsp=None, o=out, c=coc, scene=s._h):
        return lib.rt_dof(scene, ptr(src), ptr(z), C.byref(camera) if camera is not None else None,
                          C.byref(opts) if opts is not None else None, ptr(o), ptr(c))

    for call in (dev, host):
        _expect(lib, call(good), NO_DEVICE, ["host-only"])
        _expect(lib, call(good, c=None), NO_DEVICE, ["host-only"])
        _expect(lib, call(hb.dof_opts(w, h, planar_depth=0), camera=None), NO_DEVICE, ["host-only"])
        for kw in (dict(src=None), dict(z=None), dict(o=None), dict(scene=None)):
            _expect(lib, call(good, **kw), INVALID, ["null"])
        _expect(lib, call(None), INVALID, ["null"])
        for ww, hh in ((0, h), (w, 0)):
            _expect(lib, call(hb.dof_opts(ww, hh)), INVALID, ["width"])
        bad = [dict(focus_distance=0.0), dict(focus_distance=-1.0), dict(focus_distance=float("nan")), dict(focus_distance=float("inf")),
               dict(blur_scale=-0.5), dict(blur_scale=float("nan")), dict(blur_scale=float("inf")),
               dict(max_radius=0), dict(max_radius=17), dict(planar_depth=2)]
        for kw in bad:
            _expect(lib, call(hb.dof_opts(w, h, **kw)), INVALID, [next(iter(kw))])
        r = hb.dof_opts(w, h)
        r.reserved[3] = 1
        _expect(lib, call(r), INVALID, ["reserved"])
        _expect(lib, call(good, camera=None), INVALID, ["planar_depth", "camera"])  # the default wants the distance along the axis
        _expect(lib, call(hb.dof_opts(1, h)), INVALID, ["planar_depth"])  # u divides by W - 1
        _expect(lib, call(hb.dof_opts(1, 1, planar_depth=0), camera=None), NO_DEVICE, ["host-only"])
        for edge in (dict(focus_distance=1e-3), dict(blur_scale=0.0), dict(blur_scale=1e6), dict(max_radius=1), dict(max_radius=16),
                     dict(planar_depth=0)):
            _expect(lib, call(hb.dof_opts(w, h, **edge)), NO_DEVICE, ["host-only"])
        _expect(lib, call(hb.dof_opts(1 << 16, (1 << 15) + 1)), UNSUPPORTED, ["2^31"])
        # every pair of buffers, out == rgb included: this stage does not run in place
        _expect(lib, call(good, o=rgb), INVALID, ["overlap"])
        _expect(lib, call(good, o=rgb + 4), INVALID, ["overlap"])
        _expect(lib, call(good, o=rgb + 12 * n - 4), INVALID, ["overlap"])
        _expect(lib, call(good, o=rgb - 12 * n + 4), INVALID, ["overlap"])
        _expect(lib, call(good, o=depth), INVALID, ["overlap"])
        _expect(lib, call(good, z=rgb + 8), INVALID, ["overlap"])
        _expect(lib, call(good, c=rgb), INVALID, ["overlap"])
        _expect(lib, call(good, c=depth), INVALID, ["overlap"])
        _expect(lib, call(good, c=out + 12 * n - 4), INVALID, ["overlap"])
        _expect(lib, call(good, c=out + 12 * n), NO_DEVICE, ["host-only"])  # right behind the output: disjoint
    # the device call's workspace
    _expect(lib, dev(good, wsp=None), INVALID, ["workspace"])
    _expect(lib, dev(good, wsp=ws + 4), INVALID, ["aligned"])
    for other in (out, rgb, depth, coc):
        _expect(lib, dev(good, wsp=(other + 15) // 16 * 16), INVALID, ["overlap"])
    _expect(lib, dev(good, c=ws + ws_bytes - 4), INVALID, ["overlap"])
    # the one-call form
    ropts = abi.default_render_opts(w, h, 2)

    def one(ro=ropts, do=good, camera=cam, o=out, scene=s._h):
        return lib.rt_render_dof(scene, C.byref(camera) if camera is not None else None, C.byref(ro) if ro is not None else None,
                                 C.byref(do) if do is not None else None, ptr(o))

    _expect(lib, one(), NO_DEVICE, ["host-only"])
    _expect(lib, one(do=hb.dof_opts(0, 0, blur_scale=2.0)), NO_DEVICE, ["host-only"])  # the sizes come from the render
    for kw in (dict(ro=None), dict(do=None), dict(camera=None), dict(o=None), dict(scene=None)):
        _expect(lib, one(**kw), INVALID, ["null"])
    _expect(lib, one(do=hb.dof_opts(w, h, max_radius=17)), INVALID, ["max_radius"])
    _expect(lib, one(ro=abi.default_render_opts(1, h, 2)), INVALID, ["planar_depth"])
    _expect(lib, one(ro=abi.default_render_opts(1, h, 2), do=hb.dof_opts(w, h, planar_depth=0)), INVALID, ["width"])
    sharded = abi.default_render_opts(w, h, 2)
    sharded.shard_count = 2
    _expect(lib, one(ro=sharded), UNSUPPORTED, ["shard_count"])
    method = abi.default_render_opts(w, h, 2)
    method.render_method = 7
    _expect(lib, one(ro=method), INVALID, ["render method"])
    # the Python wrappers
    img, z = np.zeros((h, w, 3), F32), np.ones((h, w), F32)
    with pytest.raises(hb.RtHipError) as e:
        s.dof(img, z, cam)
    assert e.value.code == NO_DEVICE
    with pytest.raises(hb.RtHipError) as e:
        s.render_dof(cam, ropts, good)
    assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        s.dof(img[..., :2], z, cam)
    with pytest.raises(ValueError):
        s.dof(img, z[1:], cam)


# ---- the checker on hand-computed cases ----
def _frame(h, w, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 1.0, (h, w, 3)) * np.exp2(rng.uniform(-6, 6, (h, w, 1)))).astype(F32)


def test_blur_scale_zero_returns_the_input_bytes():
    img = _frame(9, 14)
    img[0, 0] = (-0.0, np.finfo(F32).max, np.finfo(F32).tiny / 8)  # -0, FLT_MAX and a subnormal come back as they are
    img[3, 4] = (np.nan, 1.0, 2.0)
    img[5, 5] = (np.inf, -np.inf, 0.0)
    img[8, 13] = (-3.0, -0.0, 1e30)
    rng = np.random.default_rng(2)
    depth = rng.uniform(0.1, 40.0, (9, 14)).astype(F32)
    depth[1, 1], depth[2, 2], depth[4, 4], depth[6, 6] = 0.0, np.nan, 1e-45, -2.0  # 1e-45: |z - f| / z overflows, k is FLT_MAX
    for R in (1, 8, 16):
        out, coc = K.dof(img, depth, blur_scale=0.0, max_radius=R, planar_depth=0, coc=True)
        assert out.tobytes() == img.tobytes()
        assert (np.abs(coc) == F32(0.5)).all()
    assert K.dof(img, depth, hb_camera(), blur_scale=0.0).tobytes() == img.tobytes()


def hb_camera():
    import importlib
    return importlib.import_module("raytracing-rust_amd.hip_backend").camera_new(**CAMERA_A)


def test_circle_of_confusion_by_hand():
    f = F32(4.0)
    depth = np.array([[4.0, 2.0, 8.0, 0.0, np.inf, np.nan, -1.0, 1e30, 1.0]], F32)
    r, key, near = K.circle_of_confusion(depth, focus_distance=4.0, blur_scale=6.0, max_radius=5, planar_depth=0)
    # k: 0, |2-4|/2 = 1, |8-4|/8 = 0.5, infinity -> 1 (four times), |1e30-4|/1e30 = 1, |1-4|/1 = 3
    want = np.array([0.5, 5.0, 3.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0], F32)  # 6k clamped to [0.5, 5]
    assert r.tobytes() == want[None].tobytes()
    assert key.tobytes() == np.array([[4.0, 2.0, 8.0, INF, INF, INF, INF, 1e30, 1.0]], F32).tobytes()
    assert near.tolist() == [[False, True, False, False, False, False, False, False, True]]
    coc = K.signed_coc(depth, focus_distance=4.0, blur_scale=6.0, max_radius=5, planar_depth=0)
    assert coc.tolist() == [[0.5, -5.0, 3.0, 5.0, 5.0, 5.0, 5.0, 5.0, -5.0]]
    small = K.circle_of_confusion(depth, focus_distance=4.0, blur_scale=0.25, max_radius=5, planar_depth=0)[0]
    assert (small[0, :3] == np.array([0.5, 0.5, 0.5], F32)).all() and small[0, 8] == F32(0.75)
    assert F32(6.0) * (np.abs(F32(8.0) - f) / F32(8.0)) == F32(3.0)


def test_planar_depth_puts_a_wall_in_focus_as_a_whole():
    """a plane at distance 10 along the camera's axis: t = 10 / cosine per pixel, z = t * cosine is 10 to rounding everywhere"""
    cam = hb_camera()
    w, h = 33, 19
    cos = K.cosines(cam, w, h)
    assert cos.shape == (h, w) and (cos > 0.9).all() and (cos <= 1.0).all()
    assert cos[h // 2, w // 2] == cos.max() and cos[0, 0] < cos[h // 2, w // 2]  # the centre pixel looks down the axis
    t = (F32(10.0) / cos).astype(F32)
    planar = K.circle_of_confusion(t, cam, focus_distance=10.0, blur_scale=1000.0, max_radius=16)[0]
    radial = K.circle_of_confusion(t, focus_distance=10.0, blur_scale=1000.0, max_radius=16, planar_depth=0)[0]
    assert (planar == F32(0.5)).all()  # |z - 10| / z is a few ulps: 1000 times that stays below half a pixel
    assert radial[0, 0] > F32(2.0) and radial[h // 2, w // 2] == F32(0.5)  # the corner is 10 / cos away along its ray
    # the cosine itself, by hand, for one pixel
    o, ll, hz, vt = (np.array(getattr(cam, k)[:], F32) for k in ("origin", "lower_left", "horizontal", "vertical"))
    u, v = F32(5) / F32(w - 1), F32(1) - F32(3) / F32(h - 1)
    d = ((ll + hz * u) + vt * v) - o
    d = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    a = ((ll + hz * F32(0.5)) + vt * F32(0.5)) - o
    a = a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    assert cos[3, 5] == (d[0] * a[0] + d[1] * a[1]) + d[2] * a[2]


def _disc_cover(r, d):
    return min(max((F32(r) - d) + F32(0.5), F32(0.0)), F32(1.0))


def test_single_bright_pixel_at_infinity_gives_the_disc():
    """9 x 9, everything at infinity with r = 2 (blur_scale 2, k = 1): the output at p is w(p - q0) * c / sw(p), with
    w = cover / 16 and cover 1 up to d = sqrt(2), 0.5 at d = 2, 2.5 - sqrt(5) at d = sqrt(5), 0 from d = sqrt(8) on"""
    img = np.zeros((9, 9, 3), F32)
    c = np.array([90.0, 30.0, 6.0], F32)
    img[4, 4] = c
    depth = np.zeros((9, 9), F32)
    out, coc = K.dof(img, depth, blur_scale=2.0, max_radius=3, planar_depth=0, coc=True)
    assert (coc == F32(2.0)).all()
    assert _disc_cover(2, F32(2.0)) == F32(0.5) and _disc_cover(2, np.sqrt(F32(8))) == 0 and _disc_cover(2, F32(3)) == 0
    ramp = _disc_cover(2, np.sqrt(F32(5)))
    assert ramp == (F32(2.0) - np.sqrt(F32(5))) + F32(0.5) and 0.26 < ramp < 0.27
    total = F32(0)
    for y in range(9):
        for x in range(9):
            # p's own sums, taps in the definition's order, off-frame taps skipped; wq: the weight of the bright tap, if it covers p
            sw, wq = F32(-0.0), None
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    if not (0 <= y + dy < 9 and 0 <= x + dx < 9):
                        continue
                    cover = _disc_cover(2, np.sqrt(F32(dx * dx + dy * dy)))
                    if cover == 0:
                        continue
                    wgt = cover / (F32(4.0) * F32(4.0))
                    sw = sw + wgt
                    if (y + dy, x + dx) == (4, 4):
                        wq = wgt
            want = (wq * c) / sw if wq is not None else np.zeros(3, F32)  # the black taps add w * 0 = +0
            assert out[y, x].tobytes() == want.astype(F32).tobytes(), (y, x)
            total = total + out[y, x, 0] / c[0]
    assert out[4, 4, 0] > out[4, 6, 0] > out[5, 6, 0] > 0 and out[6, 6, 0] == 0 and out[4, 7, 0] == 0
    assert out[4, 6, 0] == out[4, 2, 0] == out[2, 4, 0] == out[6, 4, 0]  # d = 2 on every side, same sw away from the border
    # an interior pixel sees the full disc: 9 taps of cover 1, 4 of 0.5, 8 of the ramp; the centre's weight over that sum
    full = F32(9) + F32(4) * F32(0.5) + F32(8) * ramp
    assert abs(float(out[4, 4, 0] / c[0]) - 1.0 / float(full)) < 1e-6
    # energy: away from the border every sw is the same, so the spread weights sum to 1 to within the rounding of 21 divisions
    assert abs(float(total) - 1.0) < 21 * 2.0 ** -23


def test_weights_sum_to_one_on_a_constant_frame():
    """out = sc / sw with every c equal: c to within the rounding of the sums (at most 49 terms at R = 3) and the division"""
    img = np.full((11, 12, 3), 0.7, F32)
    rng = np.random.default_rng(3)
    depth = rng.uniform(0.5, 30.0, (11, 12)).astype(F32)
    out = K.dof(img, depth, focus_distance=5.0, blur_scale=4.0, max_radius=3, planar_depth=0)
    assert np.abs(out / F32(0.7) - 1).max() < 50 * 2.0 ** -23


def test_a_sharp_near_pixel_keeps_its_bytes_next_to_a_blurred_far_region():
    """one pixel at the focus distance (r = 0.5) in a field far behind it (r = 4): min(r[q], r[p]) shrinks every far tap to the
    near pixel's own radius, so only its own tap covers it"""
    img = _frame(9, 9, seed=4)
    depth = np.full((9, 9), 100.0, F32)
    depth[4, 4] = 2.0
    opts = dict(focus_distance=2.0, blur_scale=4.2, max_radius=4, planar_depth=0)
    r, key, near = K.circle_of_confusion(depth, **opts)
    assert r[4, 4] == F32(0.5) and r[0, 0] == F32(4.0) and key[4, 4] < key[0, 0] and not near.any()
    out = K.dof(img, depth, **opts)
    assert out[4, 4].tobytes() == img[4, 4].tobytes()
    assert out[4, 5].tobytes() != img[4, 5].tobytes()  # its far neighbours are blurred
    # and the sharp near pixel, being sharp, gives nothing to them: the far pixel next to it sees the same sums without it
    dark = img.copy()
    dark[4, 4] = 0.0
    assert K.dof(dark, depth, **opts)[4, 5].tobytes() == out[4, 5].tobytes()


def test_a_blurred_near_pixel_spreads_over_a_sharp_far_one():
    img = np.zeros((9, 9, 3), F32)
    img[4, 4] = (8.0, 4.0, 2.0)
    depth = np.full((9, 9), 10.0, F32)  # the far field is in focus
    depth[4, 4] = 1.0                   # the bright pixel far in front of it: k = 9
    opts = dict(focus_distance=10.0, blur_scale=0.25, max_radius=4, planar_depth=0)
    r, key, near = K.circle_of_confusion(depth, **opts)
    assert r[4, 4] == F32(2.25) and near[4, 4] and (r[near == 0] == F32(0.5)).all()
    out = K.dof(img, depth, **opts)
    # at distance 2 the near disc covers (2.25 - 2) + 0.5 = 0.75 with weight 0.75 / 4.5^2; the far pixel's own tap has weight 1
    wq = F32(0.75) / (F32(4.5) * F32(4.5))
    want = (wq * img[4, 4]) / (F32(1.0) + wq)
    assert out[4, 6].tobytes() == want.tobytes() and (out[4, 6] > 0).all()
    assert not out[4, 7].any()  # d = 3 is beyond 2.25 + 0.5


def test_non_finite_taps_contribute_nothing_and_a_non_finite_centre_passes_through():
    img = _frame(7, 8, seed=5)
    depth = np.zeros((7, 8), F32)
    opts = dict(blur_scale=1.5, max_radius=2, planar_depth=0)
    dirty, hole = img.copy(), img.copy()
    odd = {(3, 3): (np.nan, 1.0, 2.0), (1, 6): (0.5, np.inf, 1.0), (5, 1): (1.0, 2.0, -np.inf)}
    for at, px in odd.items():
        dirty[at] = px
    out = K.dof(dirty, depth, **opts)
    for at in odd:
        assert out[at].tobytes() == dirty[at].tobytes()
    keep = np.ones((7, 8), bool)
    for at in odd:
        keep[at] = False
    assert np.isfinite(out[keep]).all()
    # the same as a frame in which those taps do not exist: by hand for the right-hand neighbour of (3, 3)
    sw, sc = F32(-0.0), np.full(3, -0.0, F32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            y, x = 3 + dy, 4 + dx
            if not (0 <= y < 7 and 0 <= x < 8) or (y, x) in odd:
                continue
            cover = _disc_cover(1.5, np.sqrt(F32(dx * dx + dy * dy)))
            if cover == 0:
                continue
            wgt = cover / (F32(3.0) * F32(3.0))
            sw, sc = sw + wgt, sc + wgt * img[y, x]
    assert out[3, 4].tobytes() == (sc / sw).astype(F32).tobytes()
