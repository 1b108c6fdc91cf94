"""AOV-guided upscaling (rt_upscale, include/rt_hip.h) without a GPU: the numpy checker (tests/upscale_checker.py) on cases with
known answers, then the ABI surface and every status code on a host-only scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scenes
import upscale_checker as U

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32


def centres(n_dst, n_src):
    """the continuous source-frame coordinate (pixel i has its centre at i) of every destination column / row, in float64"""
    return (np.arange(n_dst) + 0.5) / (n_dst - 1) * (n_src - 1) - 0.5


def checker_albedo(ys, xs, period):
    """a two-colour checker over continuous coordinates (in source pixels)"""
    cell = (np.floor(xs[None, :] / period) + np.floor(ys[:, None] / period)).astype(np.int64) & 1
    return np.where(cell[..., None] == 1, np.array([0.9, 0.2, 0.1], F32), np.array([0.1, 0.6, 0.8], F32)).astype(F32)


def half_planes(ys, xs, a, b, c):
    """True on the side a*x + b*y > c"""
    return a * xs[None, :] + b * ys[:, None] > c


# ---- the checker on cases with known answers ----
def test_constant_irradiance_under_a_checkered_albedo(O):
    h, w, H, W = 24, 40, 48, 80
    E = np.array([1.7, 0.9, 0.4], F32)
    src_albedo = checker_albedo(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), 2.5)
    dst_albedo = checker_albedo(centres(H, h), centres(W, w), 2.5)
    color = (src_albedo * E).astype(F32)
    out, stage = U.upscale(O, color, W, H, src=dict(albedo=src_albedo), dst=dict(albedo=dst_albedo))
    want = dst_albedo * E
    assert (stage == 1).all()
    assert np.abs(out / want - 1).max() <= 4 * 2.0 ** -23  # sum(w e) / sum(w) of a constant e, and c / d * d: a few ulp
    plain, plain_stage = U.upscale(O, color, W, H)
    assert (plain_stage == 1).all()
    wrong = np.abs(plain - want).max(axis=-1) > 0.1  # the stretched picture has the source's checker edges, not the destination's
    assert wrong.mean() > 0.05, wrong.mean()


@pytest.mark.parametrize("guide", ["depth", "normal"])
@pytest.mark.parametrize("line", [(1.0, -0.7, 9.3), (0.45, 1.0, 17.2), (-1.0, 0.31, -20.0)])
def test_oblique_edge_does_not_bleed(O, guide, line):
    h, w, H, W = 30, 44, 60, 88
    side_s = half_planes(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), *line)
    side_d = half_planes(centres(H, h), centres(W, w), *line)
    assert side_s.any() and not side_s.all()
    color = np.where(side_s[..., None], F32(5.0), F32(1.0)) * np.ones(3, F32)
    if guide == "depth":  # a depth step of a factor 2: far outside the relative tolerance, weight exactly 0
        src = dict(depth=np.where(side_s, F32(2.0), F32(1.0)).astype(F32))
        dst = dict(depth=np.where(side_d, F32(2.0), F32(1.0)).astype(F32))
    else:  # a crease of 90 degrees: dot == 0, powf(0, sigma) == 0
        up, right = np.array([0, 1, 0], F32), np.array([1, 0, 0], F32)
        src = dict(normal=np.where(side_s[..., None], up, right).astype(F32))
        dst = dict(normal=np.where(side_d[..., None], up, right).astype(F32))
    out, stage = U.upscale(O, color.astype(F32), W, H, src=src, dst=dst)
    want = np.where(side_d[..., None], F32(5.0), F32(1.0)) * np.ones(3, F32)
    assert np.abs(out / want - 1).max() <= 1e-6, "colour from the other side of the edge"
    # Along a STRAIGHT edge stage 2 is all but unreachable: the destination pixel lies inside the square of its four bilinear taps, so
    # one of them is on its side of any half-plane, and that tap's bilinear weight falls below 1/16 only where the edge passes
    # within a hair of a source pixel centre (0 or 1 pixel of 5280 for these lines).  What is asserted here is that whichever
    # stage ran, it ran next to the edge; test_isolated_source_pixel_reaches_stage_2_and_3 builds the input that guarantees it.
    assert set(np.unique(stage)) <= {1, 2}
    a, b, c = line
    dist = np.abs(a * centres(W, w)[None, :] + b * centres(H, h)[:, None] - c) / np.hypot(a, b)
    assert (dist[stage == 2] < 2.0).all()
    plain, _ = U.upscale(O, color.astype(F32), W, H)
    assert np.abs(plain / want - 1).max() > 0.3  # bilinear alone mixes the two sides


def test_isolated_source_pixel_reaches_stage_2_and_3(O):
    """one source pixel alone has the depth (and normal) of a destination region three source pixels wide: inside its bilinear cell
    stage 1, in the ring the 4 x 4 window adds stage 2 -- with that pixel's colour exactly, it is the only tap -- and beyond it stage 3"""
    h, w, H, W = 20, 28, 40, 56
    jq, iq = 9, 13
    rng = np.random.default_rng(11)
    color = rng.uniform(0.5, 2.0, (h, w, 3)).astype(F32)
    up, right = np.array([0, 1, 0], F32), np.array([1, 0, 0], F32)
    for guide in ("depth", "normal"):
        ys, xs = centres(H, h), centres(W, w)
        region = (np.abs(xs[None, :] - iq) < 3.2) & (np.abs(ys[:, None] - jq) < 3.2)
        if guide == "depth":
            zs = np.full((h, w), 2.0, F32)
            zs[jq, iq] = 1.0
            src, dst = dict(depth=zs), dict(depth=np.where(region, F32(1.0), F32(2.0)).astype(F32))
        else:
            ns = np.tile(right, (h, w, 1))
            ns[jq, iq] = up
            src, dst = dict(normal=ns), dict(normal=np.where(region[..., None], up, right).astype(F32))
        out, stage = U.upscale(O, color, W, H, src=src, dst=dst)
        fx, fy = U.source_position(W, w).astype(np.float64), U.source_position(H, h).astype(np.float64)
        di, dj = iq - np.floor(fx)[None, :], jq - np.floor(fy)[:, None]  # the pixel's place in each destination pixel's window
        in_cell = (di >= 0) & (di <= 1) & (dj >= 0) & (dj <= 1)
        in_window = (di >= -1) & (di <= 2) & (dj >= -1) & (dj <= 2)
        bil = np.where(di == 0, 1 - (fx - np.floor(fx))[None, :], (fx - np.floor(fx))[None, :]) * \
            np.where(dj == 0, 1 - (fy - np.floor(fy))[:, None], (fy - np.floor(fy))[:, None])
        safe = np.abs(bil - 1 / 16) > 1e-4  # (away from the threshold itself)
        want_stage = np.where(in_cell & (bil >= 1 / 16), 1, np.where(in_window, 2, 3))
        sel = region & safe
        assert np.array_equal(stage[sel], want_stage[sel])
        assert set(np.unique(stage[region])) == {1, 2, 3} and (stage[~region] != 0).all()
        two = region & (stage == 2)
        assert two.sum() >= 20
        assert np.abs(out[two] / color[jq, iq] - 1).max() <= 2.0 ** -22  # (wt * e) / wt
        three = region & (stage == 3)
        assert np.isin(out[three].reshape(-1, 3), color.reshape(-1, 3)).all()  # an unblended source pixel


def test_thin_object_absent_from_the_source_reaches_stage_3(O):
    h, w, H, W = 20, 30, 60, 90
    rng = np.random.default_rng(3)
    color = rng.uniform(0.5, 2.0, (h, w, 3)).astype(F32)
    src = dict(depth=np.full((h, w), 4.0, F32))
    d = np.full((H, W), 4.0, F32)
    d[:, 41] = 1.0  # one destination pixel wide, nearer than anything the source saw
    out, stage = U.upscale(O, color, W, H, src=src, dst=dict(depth=d))
    assert (stage[:, 41] == 3).all() and (np.delete(stage, 41, axis=1) == 1).all()
    # the nearest source pixel, unblended
    fx, fy = U.source_position(W, w)[41], U.source_position(H, h)
    i = int(np.clip(np.floor(fx) + (1 if fx - np.floor(fx) > 0.5 else 0), 0, w - 1))
    j = np.clip(np.floor(fy) + (fy - np.floor(fy) > 0.5), 0, h - 1).astype(int)
    assert np.array_equal(out[:, 41], color[j, i])


def test_invalid_source_pixels_never_contribute(O):
    h, w, H, W = 24, 32, 48, 64
    rng = np.random.default_rng(5)
    color = rng.uniform(0.5, 2.0, (h, w, 3)).astype(F32)
    albedo_s = rng.uniform(0.2, 1.0, (h, w, 3)).astype(F32)
    albedo_d = rng.uniform(0.2, 1.0, (H, W, 3)).astype(F32)
    bad = np.zeros((h, w), bool)
    bad[5, 7] = bad[5, 8] = bad[12, 20] = True
    bad[14:22, 3:11] = True  # a block: its middle has no valid tap even in the 4 x 4 window
    color[bad] = np.array([np.nan, 1.0, 1.0], F32)
    color[5, 8] = (1.0, np.inf, 1.0)
    color[12, 20] = (1.0, 1.0, -np.inf)
    for src, dst in ((None, None), (dict(albedo=albedo_s), dict(albedo=albedo_d))):
        if src is not None:  # finite, but c / d overflows under an albedo below 1: invalid too
            color[0, 0] = (3e38, 3e38, 3e38)
            bad[0, 0] = True
        out, stage = U.upscale(O, color, W, H, src=src, dst=dst)
        assert np.isfinite(out).all()
        assert set(np.unique(stage)) == {0, 1, 2}  # (stage 3 needs a guide that rejects a valid tap: the test above)
        zero = stage == 0
        assert zero[34:38, 12:16].all() and (out[zero] == 0).all()
        # which non-finite value marks a pixel makes no difference
        other = color.copy()
        other[bad] = (np.nan, np.nan, np.nan)
        out2, stage2 = U.upscale(O, other, W, H, src=src, dst=dst)
        assert np.array_equal(out, out2) and np.array_equal(stage, stage2)
        assert out.max() <= 2.0 * (1.0 if src is None else 1.0 / 0.2) * 1.0001  # no sample of the 3e38 pixel anywhere


@pytest.mark.parametrize("sizes", [((90, 160), (120, 213)), ((36, 64), (36, 64)), ((17, 33), (51, 41)), ((2, 2), (7, 5)),
                                   ((9, 16), (10, 17))])
def test_ramp_is_reproduced_and_borders_clamp(O, sizes):
    (h, w), (H, W) = sizes
    ramp = (np.arange(w, dtype=F32)[None, :] * F32(2) + np.arange(h, dtype=F32)[:, None] * F32(3) + F32(1))
    color = np.repeat(ramp[..., None], 3, axis=-1).astype(F32)
    out, stage = U.upscale(O, color, W, H)
    assert out.shape == (H, W, 3) and (stage == 1).all()
    xs, ys = np.clip(centres(W, w), 0, w - 1), np.clip(centres(H, h), 0, h - 1)  # bilinear with clamped taps: linear inside,
    want = 2 * xs[None, :] + 3 * ys[:, None] + 1                                  # constant beyond the outermost centres
    assert np.abs(out[..., 0] - want).max() <= 1e-4 * want.max()
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    # the first row and column lie before the first source centre: both taps clamp onto the same pixel.  (The last ones do not
    # reach the last source centre unless W == w: the mapping is the camera's, u = (x + 0.5) / (W - 1), not a stretch of the grid.)
    assert abs(float(out[0, 0, 0]) - float(color[0, 0, 0])) <= 1e-5 * float(color[0, 0, 0])
    if W > w:
        assert U.source_position(W, w)[0] < 0 and U.source_position(W, w)[-1] < w - 1
    if (h, w) == (H, W):  # 1 : 1 is the source up to the rounding of X'
        assert np.abs(out / color - 1).max() <= 1e-4


def test_guides_must_come_in_pairs(O):
    c = np.ones((4, 4, 3), F32)
    with pytest.raises(ValueError):
        U.upscale(O, c, 8, 8, src=dict(depth=np.ones((4, 4), F32)))


def test_powf_of_one_is_one_over_the_option_range(O):
    """equal normals (dot == 1.0f exactly) weigh 1 for any sigma_normal: the kernel needs no special case for them"""
    sig = np.concatenate([np.geomspace(1e-30, 1e30, 121), [32.0, 128.0, 3.4e38, 1e-45]]).astype(F32)
    assert (O.detmath(6, np.ones_like(sig), sig) == 1).all()
    assert (O.detmath(6, np.zeros_like(sig), sig) == 0).all()


# ---- the library without a device ----
def test_upscale_symbols_and_structs(hb):
    lib = hb.lib()
    for sym in ("rt_upscale_opts_default", "rt_upscale_device", "rt_upscale", "rt_render_upscaled"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(abi.UpscaleOpts) == abi.EXPECTED_SIZES["rt_upscale_opts"][1] == 56
    assert C.sizeof(abi.UpscaleInputs) == abi.EXPECTED_SIZES["rt_upscale_inputs"][1] == 56
    assert lib.rt_abi_version() == 2


def test_upscale_opts_default(hb):
    o = abi.UpscaleOpts()
    o.src_width, o.dst_height, o.reserved[3] = 5, 7, 9
    assert hb.lib().rt_upscale_opts_default(C.byref(o)) == abi.RT_OK
    assert (o.src_width, o.src_height, o.dst_width, o.dst_height) == (0, 0, 0, 0) and list(o.reserved) == [0] * 8
    assert o.sigma_normal == 32.0 and F32(o.depth_tolerance) == F32(0.1)
    for k, v in U.DEFAULTS.items():
        assert F32(getattr(o, k)) == F32(v), k
    assert hb.lib().rt_upscale_opts_default(None) == abi.RT_ERR_INVALID_ARGUMENT
    p = hb.upscale_opts(3, 4, 6, 8, sigma_normal=8.0)
    assert (p.src_width, p.src_height, p.dst_width, p.dst_height, p.sigma_normal) == (3, 4, 6, 8, 8.0)
    with pytest.raises(ValueError):
        hb.upscale_opts(3, 4, 6, 8, sigma=1.0)


def _expect(lib, rc, code, words):
    assert rc == code, (rc, code, lib.rt_last_error())
    msg = lib.rt_last_error().decode()
    assert all(word in msg for word in words), msg


def test_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    h, w, H, W = 5, 8, 10, 16
    n, N = h * w, H * W
    f = lambda count: np.zeros(count, np.float32)  # noqa: E731
    bufs = dict(color=f(3 * n), src_albedo=f(3 * n), src_normal=f(3 * n), src_depth=f(n), dst_albedo=f(3 * N), dst_normal=f(3 * N),
                dst_depth=f(N))
    out, stage = f(3 * N), np.zeros(N, np.uint8)
    inv, uns, nodev = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE

    def inputs(**replace):
        ins = abi.UpscaleInputs()
        for k, a in bufs.items():
            v = replace.get(k, a.ctypes.data)
            setattr(ins, k, C.cast(C.c_void_p(v), C.POINTER(C.c_float)) if v else None)
        return ins

    def dev(opts, ins="all", o=out.ctypes.data, st=stage.ctypes.data, scene=s._h):
        ins = inputs() if isinstance(ins, str) else ins
        return lib.rt_upscale_device(scene, C.byref(ins) if ins is not None else None, C.byref(opts) if opts is not None else None,
                                     C.c_void_p(o), C.c_void_p(st), C.c_void_p(0))

    def host(opts, ins="all", o=out.ctypes.data, st=stage.ctypes.data, scene=s._h):
        ins = inputs() if isinstance(ins, str) else ins
        return lib.rt_upscale(scene, C.byref(ins) if ins is not None else None, C.byref(opts) if opts is not None else None,
                              C.c_void_p(o), C.c_void_p(st))

    good = hb.upscale_opts(w, h, W, H)
    for call in (dev, host):
        _expect(lib, call(good), nodev, ["host-only"])
        _expect(lib, call(good, st=None), nodev, ["host-only"])
        no_guides = {k: None for k in bufs if k != "color"}
        _expect(lib, call(good, ins=inputs(**no_guides)), nodev, ["host-only"])
        for kw in (dict(scene=None), dict(ins=None)):
            _expect(lib, call(good, **kw), inv, ["null"])
        _expect(lib, call(None), inv, ["null"])
        _expect(lib, call(good, o=None), inv, ["out"])
        _expect(lib, call(good, ins=inputs(color=None)), inv, ["color"])
        for sizes in ((1, h, W, H), (w, 1, W, H), (0, 0, W, H), (w, h, 1, H), (1, 1, 1, 1)):
            _expect(lib, call(hb.upscale_opts(*sizes)), inv, ["must be >= 2"])
        for k in ("src_albedo", "src_normal", "src_depth", "dst_albedo", "dst_normal", "dst_depth"):
            _expect(lib, call(good, ins=inputs(**{k: None})), inv, ["both sizes"])
        for kw in (dict(sigma_normal=0.0), dict(sigma_normal=-1.0), dict(sigma_normal=float("nan")), dict(sigma_normal=float("inf")),
                   dict(depth_tolerance=0.0), dict(depth_tolerance=float("nan")), dict(depth_tolerance=float("-inf"))):
            _expect(lib, call(hb.upscale_opts(w, h, W, H, **kw)), inv, ["finite"])
        _expect(lib, call(hb.upscale_opts(w, h, W, H, sigma_normal=1e-6, depth_tolerance=1e6)), nodev, ["host-only"])
        _expect(lib, call(hb.upscale_opts(w, h, w - 1, H)), uns, ["downscaler"])
        _expect(lib, call(hb.upscale_opts(w, h, W, h - 1)), uns, ["downscaler"])
        _expect(lib, call(hb.upscale_opts(w, h, w, h)), nodev, ["host-only"])  # 1 : 1 is legal
        _expect(lib, call(hb.upscale_opts(w, h, 1 << 16, (1 << 15) + 1)), uns, ["2^31"])
        # the two buffers written against every other buffer
        for k, a in bufs.items():
            _expect(lib, call(good, o=a.ctypes.data), inv, ["overlaps"])
            _expect(lib, call(good, st=a.ctypes.data + a.nbytes - 1), inv, ["overlaps"])
        _expect(lib, call(good, o=bufs["color"].ctypes.data - 12 * N + 4), inv, ["overlaps"])
        _expect(lib, call(good, st=out.ctypes.data + 8), inv, ["overlaps"])
        shared = inputs(src_albedo=bufs["color"].ctypes.data, src_normal=bufs["color"].ctypes.data)  # inputs may share memory
        _expect(lib, call(good, ins=shared), nodev, ["host-only"])
    with pytest.raises(hb.RtHipError) as e:
        s.upscale(np.zeros((h, w, 3), F32), dst=(H, W))
    assert e.value.code == nodev
    with pytest.raises(ValueError):
        s.upscale(np.zeros((h, w, 3), F32))
    with pytest.raises(ValueError):
        s.upscale(np.zeros((h, w, 3), F32), src=dict(depth=np.zeros((h, w), F32)), dst=dict(depth=np.zeros((H + 1, W), F32), albedo=np.zeros((H, W, 3), F32)))


def test_render_upscaled_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    cam = hb.camera_new(**ls.camera_params)
    h, w, H, W = 9, 16, 18, 32
    out, out_src = np.zeros(3 * H * W, np.float32), np.zeros(3 * h * w, np.float32)
    inv, uns, nodev = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE

    def call(opts=None, sw=w, sh=h, dopts="default", uopts="default", o=out.ctypes.data, osrc=out_src.ctypes.data, scene=s._h,
             camera=cam):
        opts = abi.default_render_opts(W, H, 4) if opts is None else opts
        dopts = hb.denoise_opts(0, 0) if isinstance(dopts, str) else dopts
        uopts = hb.upscale_opts(0, 0, 0, 0) if isinstance(uopts, str) else uopts
        rays = C.c_uint64()
        return lib.rt_render_upscaled(scene, C.byref(camera) if camera is not None else None, C.byref(opts), C.c_uint32(sw),
                                      C.c_uint32(sh), C.byref(dopts) if dopts is not None else None,
                                      C.byref(uopts) if uopts is not None else None, C.c_void_p(o), C.c_void_p(osrc), C.byref(rays))

    _expect(lib, call(), nodev, ["host-only"])
    _expect(lib, call(osrc=None), nodev, ["host-only"])
    for kw in (dict(scene=None), dict(camera=None), dict(dopts=None), dict(uopts=None), dict(o=None)):
        _expect(lib, call(**kw), inv, ["null"])
    _expect(lib, call(sw=1), inv, ["must be >= 2"])
    _expect(lib, call(opts=abi.default_render_opts(W, H, 3)), inv, ["even"])
    _expect(lib, call(opts=abi.default_render_opts(W, H, 0)), inv, ["even"])
    _expect(lib, call(dopts=hb.denoise_opts(0, 0, iterations=11)), inv, ["iterations"])
    _expect(lib, call(uopts=hb.upscale_opts(0, 0, 0, 0, sigma_normal=0.0)), inv, ["finite"])
    _expect(lib, call(sw=W + 1), uns, ["downscaler"])
    _expect(lib, call(sh=H + 1), uns, ["downscaler"])
    shard = abi.default_render_opts(W, H, 4)
    shard.shard_index, shard.shard_count = 0, 2
    _expect(lib, call(opts=shard), uns, ["shard_count"])
    lay = abi.default_render_opts(W, H, 4)
    lay.output_layout = abi.RT_LAYOUT_SHARD
    _expect(lib, call(opts=lay), uns, ["FRAME"])
    _expect(lib, call(osrc=out.ctypes.data + 4), inv, ["overlaps"])
    with pytest.raises(hb.RtHipError) as e:
        s.render_upscaled(cam, abi.default_render_opts(W, H, 4), w, h)
    assert e.value.code == nodev


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() {\n'
           'rt_hip::UpscaleOptions u; u.sigma_normal = 8.0f; u.depth_tolerance = 0.2f;\n'
           'rt_upscale_opts (*f)(const rt_hip::UpscaleOptions &, uint32_t, uint32_t, uint32_t, uint32_t) = &rt_hip::upscale_opts;\n'
           'std::vector<float> (*g)(const rt_hip::Bvh &, const std::vector<float> &, const rt_hip::AovBuffers *, '
           'const rt_hip::AovBuffers *, uint32_t, uint32_t, uint32_t, uint32_t, const rt_hip::UpscaleOptions &, '
           'std::vector<uint8_t> *) = &rt_hip::upscale;\n'
           'rt_hip::Upscaled (*r)(const rt_hip::RenderOptions &, uint32_t, uint32_t, const rt_hip::SimpleCamera &, const rt_hip::Bvh &, '
           'const rt_hip::DenoiseOptions &, const rt_hip::UpscaleOptions &, uint64_t, uint64_t) = &rt_hip::render_upscaled;\n'
           '(void)f; (void)g; (void)r; (void)u; return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)
