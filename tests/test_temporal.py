"""Temporal accumulation with camera reprojection (rt_denoise_temporal, include/rt_hip.h) without a GPU: the float32 checker
(tests/temporal_checker.py) against analytic camera motions, and the ABI surface and status codes on a host-only scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scenes
import temporal_checker as T

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32


# ---- synthetic pinhole cameras and analytic depth ----
def pinhole(origin, yaw=0.0, fov=40.0, aspect=16 / 9, focus=1.0):
    """(4, 3) float32 camera rows (origin, lower_left, horizontal, vertical) looking down -z rotated by `yaw` degrees about +y"""
    t = np.radians(yaw)
    fwd = np.array([-np.sin(t), 0.0, -np.cos(t)])
    right = np.array([np.cos(t), 0.0, -np.sin(t)])
    up = np.array([0.0, 1.0, 0.0])
    hh = 2 * focus * np.tan(np.radians(fov) / 2)
    h, v = right * hh * aspect, up * hh
    o = np.asarray(origin, np.float64)
    ll = o + fwd * focus - h / 2 - v / 2
    return np.array([o, ll, h, v], F32)


def centre_rays(cam, w, h):
    """float64 unit directions (H, W, 3) of the pixel centres (the header's u, v)"""
    o, ll, hv, vv = (np.asarray(r, np.float64) for r in cam)
    u = (np.arange(w) + 0.5) / (w - 1)
    v = 1 - (np.arange(h) + 0.5) / (h - 1)
    d = ll + hv * u[None, :, None] + vv * v[:, None, None] - o
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def plane_depth(cam, w, h, z_plane):
    """distance to the plane z = z_plane along each centre ray (0 where it is not in front)"""
    d = centre_rays(cam, w, h)
    t = (z_plane - float(cam[0][2])) / d[..., 2]
    return np.where(t > 0, t, 0.0).astype(F32)


def run_sequence(cams, colors, depths, normals=None, **opts):
    """the checker over a sequence, feeding each step's history (H0.rgb = e: no filter in between) to the next"""
    hist, prev, out = None, None, []
    for i, cam in enumerate(cams):
        st = T.step(colors[i], depths[i], cam, prev, hist, normal=None if normals is None else normals[i], **opts)
        out.append(st)
        hist, prev = st["history"], cam
    return out


W, H = 48, 27


def test_static_camera_counts_and_running_moments():
    cam = pinhole((0, 0, 0))
    z = plane_depth(cam, W, H, -5.0)
    levels = [0.3, 0.7, 0.2, 0.9, 0.5, 0.4, 0.8, 0.6]
    colors = [np.full((H, W, 3), c, F32) for c in levels]
    seq = run_sequence([cam] * len(levels), colors, [z] * len(levels))
    m1_ref = m2_ref = None
    for t, (st, c) in enumerate(zip(seq, levels)):
        n = t + 1
        assert np.array_equal(st["n"], np.full((H, W), n, F32)), t
        if t == 0:
            assert np.isnan(st["motion"]).all()
        else:
            assert np.abs(st["motion"]).max() < 1e-3
        l = float(T.lum32(np.array([c, c, c], F32)))
        a = max(0.2, 1.0 / n)
        m1_ref = l if t == 0 else m1_ref + a * (l - m1_ref)
        m2_ref = l * l if t == 0 else m2_ref + a * (l * l - m2_ref)
        assert np.allclose(st["m1"], m1_ref, rtol=1e-5) and np.allclose(st["m2"], m2_ref, rtol=1e-5), t
        # the moments' variance takes over at n = 4
        expect = max(0.0, m2_ref - m1_ref * m1_ref) if n >= 4 else 0.0
        assert np.allclose(st["var"], expect, atol=1e-5), t


def test_max_history_caps_n():
    cam = pinhole((0, 0, 0))
    z = plane_depth(cam, W, H, -5.0)
    c = np.full((H, W, 3), 0.5, F32)
    seq = run_sequence([cam] * 6, [c] * 6, [z] * 6, max_history=3)
    assert [float(s["n"].max()) for s in seq] == [1, 2, 3, 3, 3, 3]


def test_translation_over_a_fronto_parallel_plane_shifts_analytically():
    dx, zp = 0.3, -4.0
    cams = [pinhole((0, 0, 0)), pinhole((dx, 0, 0))]
    zs = [plane_depth(c, W, H, zp) for c in cams]
    c = np.full((H, W, 3), 0.5, F32)
    seq = run_sequence(cams, [c, c], zs)
    m = seq[1]["motion"]
    # the camera moves right by dx: a point at depth |zp| was dx / (pixel pitch at that depth) pixels further right before
    pitch = np.linalg.norm(cams[0][2].astype(np.float64)) * abs(zp) / 1.0 / (W - 1)
    assert np.allclose(m[..., 0], dx / pitch, atol=1e-3) and dx / pitch > 2
    assert np.abs(m[..., 1]).max() < 1e-3
    n = seq[1]["n"]
    fx = np.arange(W)[None, :] + m[..., 0]  # X' - 0.5
    assert (n[fx <= W - 2] == 2).all()  # both columns of taps in the old frame
    assert (n[fx >= W] == 1).all() and (fx >= W).any()  # reprojected out of the old frame


def _step_scene(cam, w, h):
    """a foreground half plane x < 0 at z = -2 in front of a background plane at z = -8: (depth, is_foreground)"""
    d = centre_rays(cam, w, h)
    o = cam[0].astype(np.float64)
    t_fg = (-2.0 - o[2]) / d[..., 2]
    x_fg = o[0] + t_fg * d[..., 0]
    fg = (t_fg > 0) & (x_fg < 0)
    t_bg = (-8.0 - o[2]) / d[..., 2]
    return np.where(fg, t_fg, t_bg).astype(F32), fg


def test_depth_step_disocclusion_restarts_history():
    w, h = 96, 54
    cams = [pinhole((0, 0, 0)), pinhole((0.3, 0, 0))]
    (z0, _), (z1, fg1) = _step_scene(cams[0], w, h), _step_scene(cams[1], w, h)
    c = np.full((h, w, 3), 0.5, F32)
    seq = run_sequence(cams, [c, c], [z0, z1])
    n = seq[1]["n"]
    # where was each background point of frame 1 seen from camera 0?  occluded iff the segment to it crosses x < 0 at z = -2
    d = centre_rays(cams[1], w, h)
    o1, o0 = cams[1][0].astype(np.float64), cams[0][0].astype(np.float64)
    p = o1 + d * z1[..., None].astype(np.float64)
    s = (-2.0 - o0[2]) / (p[..., 2] - o0[2])
    x_cross = o0[0] + s * (p[..., 0] - o0[0])
    occluded = ~fg1 & (x_cross < 0)
    # keep away from the silhouettes (2 px) and the frame's left edge, where bilinear taps straddle
    far = np.ones_like(fg1)
    for sh in range(-2, 3):
        far &= np.roll(fg1, sh, axis=1) == fg1
        far &= np.roll(occluded, sh, axis=1) == occluded
    far[:, :8] = False
    assert (occluded & far).sum() > 20 and (~occluded & ~fg1 & far).sum() > 20
    assert (n[occluded & far] == 1).all()  # the disoccluded side: no history
    assert (n[~occluded & far] == 2).all()  # foreground and visible background keep theirs


def test_pure_rotation_moves_the_sky_by_direction():
    cams = [pinhole((1, 2, 3), yaw=0.0), pinhole((1, 2, 3), yaw=2.0)]
    z = np.zeros((H, W), F32)  # all sky
    c = np.full((H, W, 3), 0.25, F32)
    seq = run_sequence(cams, [c, c], [z, z])
    # each direction of camera 1 expressed in camera 0's image
    d = centre_rays(cams[1], W, H)
    o, ll, hv, vv = (r.astype(np.float64) for r in cams[0])
    m = np.stack([ll - o, hv, vv], axis=1)  # columns: d = s*(ll - o) + a*h + b*v
    sol = np.linalg.solve(m, d.reshape(-1, 3).T).T.reshape(H, W, 3)
    x_ref = sol[..., 1] / sol[..., 0] * (W - 1) - (np.arange(W) + 0.5)[None, :]
    y_ref = (1 - sol[..., 2] / sol[..., 0]) * (H - 1) - (np.arange(H) + 0.5)[:, None]
    got = seq[1]["motion"]
    assert np.allclose(got[..., 0], x_ref, atol=2e-3) and np.allclose(got[..., 1], y_ref, atol=2e-3)
    assert np.abs(got[..., 0]).min() > 1.0  # it really moved
    assert (seq[1]["n"][:, 4:] == 2).all()


def test_point_behind_the_previous_camera_has_no_motion():
    cams = [pinhole((0, 0, 0), yaw=180.0), pinhole((0, 0, 0))]
    z0 = np.full((H, W), 3.0, F32)
    z1 = plane_depth(cams[1], W, H, -5.0)
    c = np.full((H, W, 3), 0.5, F32)
    seq = run_sequence(cams, [c, c], [z0, z1])
    assert np.isnan(seq[1]["motion"]).all()
    assert (seq[1]["n"] == 1).all()


def test_invalid_pixels_write_n_zero_and_are_never_taps():
    cam = pinhole((0, 0, 0))
    z = plane_depth(cam, W, H, -5.0)
    c = np.full((H, W, 3), 0.5, F32)
    bad = c.copy()
    bad[5, 7, 1] = np.nan
    bad[9, 20, 0] = np.inf
    s0 = T.step(bad, z, cam)
    assert s0["n"][5, 7] == 0 and s0["n"][9, 20] == 0 and not s0["valid"][5, 7]
    s1 = T.step(c, z, cam, cam, s0["history"])
    assert s1["n"][5, 7] == 1 and s1["n"][9, 20] == 1  # its own old pixel was not a tap
    assert (np.delete(s1["n"].ravel(), [5 * W + 7, 9 * W + 20]) == 2).all()


def test_normal_rejection():
    cam = pinhole((0, 0, 0))
    z = plane_depth(cam, W, H, -5.0)
    c = np.full((H, W, 3), 0.5, F32)
    n0 = np.zeros((H, W, 3), F32)
    n0[..., 2] = 1
    n1 = n0.copy()
    n1[:, : W // 2] = (1, 0, 0)  # turned by 90 degrees on the left half
    seq = run_sequence([cam, cam], [c, c], [z, z], normals=[n0, n1])
    assert (seq[1]["n"][:, : W // 2] == 1).all() and (seq[1]["n"][:, W // 2:] == 2).all()
    seq = run_sequence([cam, cam], [c, c], [z, z], normals=[n0, n1], normal_tolerance=-1.0)
    assert (seq[1]["n"] == 2).all()


def test_constant_image_stays_constant():
    cams = [pinhole((0.02 * i, 0, 0), yaw=0.3 * i) for i in range(5)]
    zs = [plane_depth(cm, W, H, -5.0) for cm in cams]
    c = np.full((H, W, 3), (0.3, 0.5, 0.7), F32)
    hist, prev = None, None
    for cm, z in zip(cams, zs):
        st = T.step(c, z, cm, prev, hist)
        e1, out = T.filtered(st, c, False, iterations=3)
        assert np.allclose(out, c, rtol=1e-6, atol=0), np.abs(out - c).max()
        hist = st["history"].copy()
        hist[0, ..., :3] = e1
        prev = cm


# ---- the library without a device ----
def test_temporal_symbols_and_structs(hb):
    lib = hb.lib()
    for sym in ("rt_temporal_opts_default", "rt_temporal_history_bytes", "rt_temporal_workspace_bytes", "rt_denoise_temporal_device",
                "rt_denoise_temporal", "rt_denoise_temporal_reset"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(abi.TemporalOpts) == abi.EXPECTED_SIZES["rt_temporal_opts"][1] == 96
    assert C.sizeof(abi.TemporalInputs) == abi.EXPECTED_SIZES["rt_temporal_inputs"][1] == 32
    assert tuple(n for n, _ in abi.TemporalInputs._fields_) == abi.TEMPORAL_INPUTS


def test_temporal_opts_default(hb):
    o = abi.TemporalOpts()
    o.max_history, o.reserved[3], o.denoise.width = 9, 5, 7
    assert hb.lib().rt_temporal_opts_default(C.byref(o)) == abi.RT_OK
    assert (o.denoise.width, o.denoise.height, o.denoise.iterations) == (0, 0, 5)
    assert (o.denoise.sigma_luminance, o.denoise.sigma_normal) == (4.0, 128.0)
    assert o.denoise.sigma_depth == F32(0.1)
    assert (o.alpha_color, o.alpha_moments, o.depth_tolerance, o.normal_tolerance) == (F32(0.2), F32(0.2), F32(0.1), F32(0.9))
    assert o.max_history == 32 and list(o.reserved) == [0] * 7 and list(o.denoise.reserved) == [0] * 6
    assert hb.lib().rt_temporal_opts_default(None) == abi.RT_ERR_INVALID_ARGUMENT
    p = hb.temporal_opts(3, 4, iterations=2, max_history=8, alpha_color=0.5)
    assert (p.denoise.width, p.denoise.height, p.denoise.iterations, p.max_history, p.alpha_color) == (3, 4, 2, 8, 0.5)
    with pytest.raises(ValueError):
        hb.temporal_opts(3, 4, alpha=0.5)


@pytest.mark.parametrize("w,h", [(2, 2), (64, 36), (67, 37), (1920, 1080), (1 << 16, 1 << 15)])
def test_history_and_workspace_bytes(hb, w, h):
    o = hb.temporal_opts(w, h)
    assert hb.temporal_history_bytes(o) == 48 * w * h == abi.TEMPORAL_HISTORY_BYTES_PER_PIXEL * w * h
    assert hb.temporal_workspace_bytes(o) == 32 * w * h == abi.TEMPORAL_WORKSPACE_BYTES_PER_PIXEL * w * h


def test_bytes_reject(hb):
    lib = hb.lib()
    n = C.c_uint64()
    for fn in (lib.rt_temporal_history_bytes, lib.rt_temporal_workspace_bytes):
        for w, h in ((1, 5), (5, 1), (0, 0)):
            assert fn(C.byref(hb.temporal_opts(w, h)), C.byref(n)) == abi.RT_ERR_INVALID_ARGUMENT
        assert fn(C.byref(hb.temporal_opts(1 << 16, (1 << 15) + 1)), C.byref(n)) == abi.RT_ERR_UNSUPPORTED
        assert fn(None, C.byref(n)) == abi.RT_ERR_INVALID_ARGUMENT


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
    cam = hb.camera_new(**ls.camera_params)
    lib = hb.lib()
    h, w = 9, 16
    n = h * w
    arrays = {k: np.zeros((h, w, 3) if k != "depth" else (h, w), np.float32) for k in abi.TEMPORAL_INPUTS}
    ins = abi.TemporalInputs()
    for k, a in arrays.items():
        setattr(ins, k, a.ctypes.data_as(C.POINTER(C.c_float)))
    out = np.zeros((h, w, 3), np.float32)
    motion = np.zeros((h, w, 2), np.float32)
    out_p, mo_p = out.ctypes.data_as(C.POINTER(C.c_float)), motion.ctypes.data_as(C.POINTER(C.c_float))
    k1, h_in = _aligned(48 * n)
    k2, h_out = _aligned(48 * n)
    k3, ws = _aligned(32 * n)
    fp = lambda a: C.cast(C.c_void_p(a), C.POINTER(C.c_float))  # noqa: E731
    inv = abi.RT_ERR_INVALID_ARGUMENT

    def dev(opts, inputs=ins, cam_=cam, prev=cam, hin=h_in, hout=h_out, wsp=ws, o=out_p, m=mo_p):
        return lib.rt_denoise_temporal_device(s._h, C.byref(inputs), C.byref(cam_) if cam_ is not None else None,
                                              C.byref(prev) if prev is not None else None, C.c_void_p(hin), C.c_void_p(hout),
                                              C.byref(opts), C.c_void_p(wsp), o, m, C.c_void_p(0))

    def host(opts, inputs=ins, o=out_p, m=mo_p):
        return lib.rt_denoise_temporal(s._h, C.byref(inputs), C.byref(cam), C.byref(opts), o, m)

    good = hb.temporal_opts(w, h)
    for call in (dev, host):
        _expect(lib, call(good), abi.RT_ERR_NO_DEVICE, ["host-only"])
        _expect(lib, call(good, m=None), abi.RT_ERR_NO_DEVICE, ["host-only"])
        for missing in ("color", "depth"):
            partial = abi.TemporalInputs()
            for k in abi.TEMPORAL_INPUTS:
                if k != missing:
                    setattr(partial, k, getattr(ins, k))
            _expect(lib, call(good, inputs=partial), inv, ["depth"])
        only = abi.TemporalInputs()
        only.color, only.depth = ins.color, ins.depth
        _expect(lib, call(good, inputs=only), abi.RT_ERR_NO_DEVICE, ["host-only"])
        _expect(lib, call(good, o=None), inv, ["out"])
        for ww, hh in ((1, h), (w, 1), (0, 0)):
            _expect(lib, call(hb.temporal_opts(ww, hh)), inv, ["width"])
        bad_opts = [dict(iterations=0), dict(iterations=11), dict(sigma_depth=0.0), dict(alpha_color=0.0), dict(alpha_color=1.5),
                    dict(alpha_moments=float("nan")), dict(alpha_moments=-0.1), dict(depth_tolerance=0.0),
                    dict(depth_tolerance=float("inf")), dict(depth_tolerance=float("nan")), dict(normal_tolerance=1.01),
                    dict(normal_tolerance=-1.5), dict(normal_tolerance=float("nan")), dict(max_history=0)]
        for kw in bad_opts:
            assert call(hb.temporal_opts(w, h, **kw)) == inv, kw
        for edge in (dict(alpha_color=1.0, alpha_moments=1.0), dict(normal_tolerance=-1.0), dict(normal_tolerance=1.0),
                     dict(max_history=1)):
            _expect(lib, call(hb.temporal_opts(w, h, **edge)), abi.RT_ERR_NO_DEVICE, ["host-only"])
        _expect(lib, call(hb.temporal_opts(1 << 16, (1 << 15) + 1)), abi.RT_ERR_UNSUPPORTED, ["2^31"])
        for k in abi.TEMPORAL_INPUTS:  # out or motion aliasing an input
            _expect(lib, call(good, o=C.cast(getattr(ins, k), C.POINTER(C.c_float))), inv, ["overlaps"])
            _expect(lib, call(good, m=C.cast(getattr(ins, k), C.POINTER(C.c_float))), inv, ["overlaps"])
        _expect(lib, call(good, m=out_p), inv, ["overlaps"])
    # the device call's own buffers
    _expect(lib, dev(good, hin=h_out), inv, ["overlaps"])
    _expect(lib, dev(good, hin=h_out + 16), inv, ["overlaps"])
    _expect(lib, dev(good, wsp=h_out), inv, ["overlaps"])
    _expect(lib, dev(good, hout=(arrays["albedo"].ctypes.data + 15) // 16 * 16), inv, ["overlaps"])
    _expect(lib, dev(good, o=fp(h_in)), inv, ["overlaps"])
    _expect(lib, dev(good, m=fp(ws)), inv, ["overlaps"])
    for kw in (dict(hin=h_in + 4), dict(hout=h_out + 8), dict(wsp=ws + 4)):
        _expect(lib, dev(good, **kw), inv, ["aligned"])
    _expect(lib, dev(good, hout=0), inv, ["history_out"])
    _expect(lib, dev(good, wsp=0), inv, ["workspace"])
    _expect(lib, dev(good, prev=None), inv, ["previous camera"])
    _expect(lib, dev(good, prev=None, hin=0), abi.RT_ERR_NO_DEVICE, ["host-only"])  # no history: prev_cam unused
    _expect(lib, dev(good, cam_=None), inv, ["null"])
    assert lib.rt_denoise_temporal(None, C.byref(ins), C.byref(cam), C.byref(good), out_p, mo_p) == inv
    # reset needs no device
    assert lib.rt_denoise_temporal_reset(s._h) == abi.RT_OK
    assert lib.rt_denoise_temporal_reset(None) == inv
    s.temporal_reset()
    with pytest.raises(hb.RtHipError) as e:
        s.denoise_temporal(out, cam, depth=arrays["depth"])
    assert e.value.code == abi.RT_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        s.denoise_temporal(out, cam)
    with pytest.raises(ValueError):
        s.denoise_temporal(out, cam, depth=np.zeros((h + 1, w), np.float32))


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() {\n'
           'rt_hip::TemporalOptions t; t.denoise.iterations = 3; t.alpha_color = 0.1f;\n'
           'rt_temporal_opts (*f)(const rt_hip::TemporalOptions &, uint32_t, uint32_t) = &rt_hip::temporal_opts;\n'
           'std::vector<float> (rt_hip::TemporalDenoiser::*g)(const std::vector<float> &, const rt_hip::AovBuffers &,'
           ' const rt_hip::SimpleCamera &, std::vector<float> *) = &rt_hip::TemporalDenoiser::operator();\n'
           'void (rt_hip::TemporalDenoiser::*r)() = &rt_hip::TemporalDenoiser::reset;\n'
           '(void)f; (void)g; (void)r; (void)t; return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)
