"""The off-default option values of the post-processing stages and the synthetic inputs they run on: ONE table for
tests/test_post_options.py (CPU: every value must change the checker's result on its input, or the GPU comparison proves nothing)
and tests/test_gpu_post_options.py (GPU: the kernels and both entry points against the checker at that value).

A case is (id, options) or (id, input key, options).  Unless noted a case moves ONE option, and every option has a value on each
side of its default.  Exceptions, each because no input makes the other side observable:
  display ev_max   target = key_ev - metered and metered >= -16 (bin 0), so at the default key_ev the target never passes 13.6: a
                   value above the default 16 changes nothing.  Both values are below it; the combined case raises key_ev as well
                   and has ev_max = 18 clamp a target of 18.9 there.
"""
import numpy as np

import denoise_checker as K
import display_checker as D
import temporal_checker as T
import upscale_checker as U
from post_runners import TOL, synthetic

F32 = np.float32
SENSITIVITY = 100 * TOL  # what an option must move the checker by, in denoise_checker.relative_error, to count as exercised
SIGMAS = ("sigma_luminance", "sigma_normal", "sigma_depth")

# ---- rt_denoise / rt_denoise_device / rt_render_denoised: defaults 4, 128, 0.1 ----
DENOISE_CASES = [
    ("sigma_luminance_low", dict(sigma_luminance=1.0)),
    ("sigma_luminance_high", dict(sigma_luminance=16.0)),
    ("sigma_normal_low", dict(sigma_normal=8.0)),
    ("sigma_normal_high", dict(sigma_normal=512.0)),
    ("sigma_depth_low", dict(sigma_depth=0.02)),
    ("sigma_depth_high", dict(sigma_depth=0.5)),
    ("all", dict(sigma_luminance=1.5, sigma_normal=16.0, sigma_depth=0.3, iterations=3)),
]
DENOISE_RENDERED = ("rtweekend1", 67, 37)  # (a name of post_runners.SCENES, w, h): the GPU test checks sensitivity itself


def denoise_synthetic():
    """post_runners.synthetic at 67 x 37: random normals and depths, so the normal and depth weights matter"""
    return synthetic(37, 67, seed=5)


def denoise_sensitivity(inputs, opts):
    """how far `opts` move the checker away from its result at the defaults on `inputs`"""
    args = (inputs["color"], inputs.get("albedo"), inputs.get("normal"), inputs.get("depth"), inputs.get("variance"))
    return K.relative_error(K.denoise(*args, **opts), K.denoise(*args))


# ---- rt_denoise_temporal[_device]: defaults 0.2, 0.2, 0.1, 0.9, 32 and the three sigmas ----
# (id, sequence, frames, options).  "moving": a camera that translates and turns; "static": one camera, constant guides.
# alpha = max(alpha_x, 1 / n): a value BELOW the default 0.2 first shows at n = 6, hence the 7-frame sequences.  max_history above
# the default shows in n alone (alpha's 1 / n is long below 0.2 by then), at frame 33; the sequence runs past the cap of 36.
TEMPORAL_SIZE = (40, 23)
TEMPORAL_STATIC_SIZE = (24, 14)
TEMPORAL_ITERATIONS = 2
TEMPORAL_CASES = [
    ("alpha_color_low", "moving", 7, dict(alpha_color=0.05)),
    ("alpha_color_high", "moving", 3, dict(alpha_color=0.6)),
    ("alpha_moments_low", "moving", 7, dict(alpha_moments=0.05)),
    ("alpha_moments_high", "moving", 3, dict(alpha_moments=0.6)),
    ("depth_tolerance_low", "moving", 3, dict(depth_tolerance=0.02)),
    ("depth_tolerance_high", "moving", 3, dict(depth_tolerance=0.4)),
    ("normal_tolerance_low", "moving", 3, dict(normal_tolerance=0.5)),
    ("normal_tolerance_high", "moving", 3, dict(normal_tolerance=0.99)),
    ("max_history_low", "static", 4, dict(max_history=2)),
    ("max_history_high", "static", 38, dict(max_history=36)),
    ("sigma_luminance_low", "moving", 3, dict(sigma_luminance=1.0)),
    ("sigma_luminance_high", "moving", 3, dict(sigma_luminance=16.0)),
    ("sigma_normal_low", "moving", 3, dict(sigma_normal=8.0)),
    ("sigma_normal_high", "moving", 3, dict(sigma_normal=512.0)),
    ("sigma_depth_low", "moving", 3, dict(sigma_depth=0.02)),
    ("sigma_depth_high", "moving", 3, dict(sigma_depth=0.5)),
    ("all", "moving", 7, dict(alpha_color=0.1, alpha_moments=0.4, depth_tolerance=0.25, normal_tolerance=0.7, max_history=4,
                             sigma_luminance=2.0, sigma_normal=32.0, sigma_depth=0.3)),
]


def temporal_camera(hb, kind, i):
    k = i if kind == "moving" else 0
    return hb.camera_new(origin=(0.06 * k, 0.02 * k, 0.0), lookat=(0.0, 0.0, -5.0), vup=(0.0, 1.0, 0.0), fov=40.0, aspect_ratio=16 / 9,
                         aperture=0.0, focus_dist=1.0)


def temporal_frame(kind, i):
    """frame i of a sequence: color and albedo new every frame.  "moving": depths scattered +-25 % about 5 and normals scattered
    about +z, new every frame, so that every depth and normal tolerance of the table accepts some taps and rejects others; a patch
    of sky (z = 0), a zero normal and two non-finite pixels.  "static": constant depth and normal (every tap accepted)."""
    w, h = TEMPORAL_SIZE if kind == "moving" else TEMPORAL_STATIC_SIZE
    rng = np.random.default_rng(1000 + i)
    f = dict(color=rng.uniform(0.0, 2.0, (h, w, 3)).astype(F32), albedo=rng.uniform(0.1, 1.0, (h, w, 3)).astype(F32))
    if kind == "moving":
        n = np.array([0, 0, 1], F32) + F32(0.45) * rng.normal(size=(h, w, 3)).astype(F32)
        z = (F32(5.0) * (F32(1) + rng.uniform(-0.25, 0.25, (h, w)))).astype(F32)
        z[:3, :5] = 0
        n[:3, :5] = 0
        n[10, 10] = 0
        f["color"][7, 9, 1] = np.nan
        f["color"][15, 30, 0] = np.inf
    else:
        n = np.tile(np.array([0, 0, 1], F32), (h, w, 1))
        z = np.full((h, w), 5.0, F32)
    return dict(f, normal=n.astype(F32), depth=z)


def temporal_checker_sequence(hb, kind, frames, opts):
    """the checker alone over a sequence: each step's history carries e_1 of the checker's own filter.  Returns the last frame's
    (out, e, n, m1, m2), what a GPU run is compared on."""
    hist = prev = None
    sig = {k: v for k, v in opts.items() if k in SIGMAS}
    for i in range(frames):
        cam, f = temporal_camera(hb, kind, i), temporal_frame(kind, i)
        st = T.step(f["color"], f["depth"], cam, prev, hist, albedo=f["albedo"], normal=f["normal"], **opts)
        e1, out = T.filtered(st, f["color"], True, iterations=TEMPORAL_ITERATIONS, **sig)
        hist = st["history"].copy()
        hist[0, ..., :3] = e1.astype(F32)
        prev = cam
    ok = st["valid"]
    return dict(out=out[ok], e=st["e"][ok], n=st["n"][ok], m1=st["m1"][ok], m2=st["m2"][ok])


def temporal_sensitivity(hb, kind, frames, opts):
    """the largest relative_error between the checker at `opts` and at the defaults over the last frame's out and history planes"""
    a, b = temporal_checker_sequence(hb, kind, frames, opts), temporal_checker_sequence(hb, kind, frames, {})
    return {k: K.relative_error(a[k], b[k]) for k in a}


# ---- rt_display[_device]: defaults key_ev log2(0.18), meter window 0.10 .. 0.90, ev_min -16, ev_max 16 ----
DISPLAY_CASES = [
    ("key_ev_low", "mid", dict(key_ev=-4.0)),
    ("key_ev_high", "mid", dict(key_ev=-1.0)),
    ("meter_low_zero", "mid", dict(meter_low=0.0)),
    ("meter_low_high", "mid", dict(meter_low=0.45)),
    ("meter_high_low", "mid", dict(meter_high=0.55)),
    ("meter_high_one", "mid", dict(meter_high=1.0)),
    ("meter_whole", "mid", dict(meter_low=0.0, meter_high=1.0)),
    ("meter_narrow", "mid", dict(meter_low=0.48, meter_high=0.52)),
    ("ev_min_clamps", "mid", dict(ev_min=0.5)),  # the target is about -0.54: clamped up to 0.5
    ("ev_min_lower", "bright", dict(ev_min=-20.0)),  # the target is about -16.3: the default clamps it, this does not
    ("ev_max_clamps", "dark", dict(ev_max=1.0)),  # the target is about +10.4
    ("ev_max_clamps_less", "dark", dict(ev_max=8.0)),
    ("all", "dark", dict(key_ev=6.0, meter_low=0.3, meter_high=0.6, ev_min=-3.0, ev_max=18.0, white=3.0, gamma=1.8, seed=99,
                         adaptation=0.5, exposure_ev=0.25)),
]
DISPLAY_STATES = (("zero state", (F32(0), 0, F32(0))), ("adapting", (F32(1.25), 5, F32(-3.0))))


def display_image(key):
    """33 x 17, luminances spread over ten octaves (so a metering window cuts into the histogram), with unmetered pixels"""
    rng = np.random.default_rng(77)
    img = (rng.uniform(0.2, 1.0, (17, 33, 3)) * 2.0 ** rng.uniform(-6.0, 4.0, (17, 33, 1))).astype(F32)
    img.ravel()[:4] = [np.nan, np.inf, 0.0, -1.0]
    img[5, 5] = 0
    return img * F32({"mid": 1.0, "bright": 2.0 ** 16, "dark": 2.0 ** -11}[key])


def display_differs(O, img, state, opts):
    """does the checker's result (bytes or state) at `opts` differ from the one at the defaults?"""
    # the options that are not under test here keep the value the case gives them on both sides
    fixed = {k: v for k, v in opts.items() if k not in ("key_ev", "meter_low", "meter_high", "ev_min", "ev_max")}
    px, _, st = D.display(O, img, state, **opts)
    px0, _, st0 = D.display(O, img, state, **fixed)
    return bool((px != px0).any()), st[0] != st0[0]


# ---- rt_upscale / rt_upscale_device / rt_render_upscaled: defaults 32, 0.1 ----
UPSCALE_CASES = [
    ("sigma_normal_low", dict(sigma_normal=4.0)),
    ("sigma_normal_high", dict(sigma_normal=256.0)),
    ("depth_tolerance_low", dict(depth_tolerance=0.02)),
    ("depth_tolerance_high", dict(depth_tolerance=0.5)),
    ("all", dict(sigma_normal=8.0, depth_tolerance=0.3)),
]
UPSCALE_RENDERED = ("all_materials", (64, 36), (128, 72))  # the GPU test checks sensitivity itself


def upscale_synthetic():
    """a frame with smoothly varying normals and depths at both sizes (so both options weigh every tap)"""
    rng = np.random.default_rng(31)
    h, w, H, W = 20, 28, 40, 56

    def guides(hh, ww):
        y, x = np.meshgrid(np.linspace(0, 1, hh), np.linspace(0, 1, ww), indexing="ij")
        n = np.stack([np.sin(9 * x), np.cos(7 * y), 0.4 + 0 * x], axis=-1)
        return dict(albedo=(0.2 + 0.6 * np.stack([x, y, 1 - x], axis=-1)).astype(F32), normal=n.astype(F32),
                    depth=(2.0 + np.sin(6 * x + 4 * y) * 0.6).astype(F32))

    return rng.uniform(0.2, 2.0, (h, w, 3)).astype(F32), guides(h, w), guides(H, W), W, H


UPSCALE_SYNTHETIC = {"smooth": upscale_synthetic}


def upscale_differs(O, color, src, dst, W, H, opts):
    out, stage = U.upscale(O, color, W, H, src=src, dst=dst, **opts)
    out0, stage0 = U.upscale(O, color, W, H, src=src, dst=dst)
    return out.tobytes() != out0.tobytes() or stage.tobytes() != stage0.tobytes()
