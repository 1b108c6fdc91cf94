"""Frames past every grid cap of the post-processing kernels, so that each grid-stride loop runs a second pass:
  65 536 tiles of 16 x 16   denoise_variance_kernel, denoise_iteration_kernel<LAST> and <!LAST>: 1 x 1 048 577 (65 537 tiles),
                            17 x 524 300 (two tile columns, the second one an edge tile: 65 538 tiles), 16 x 1 048 592
  16 777 216 pixels         denoise_prepass_kernel<0 / 1 / 2>, temporal_resolve, temporal_feedback: 16 x 1 048 592
  8 388 608 / 4 194 304 px  display_map<true> / <false>: 4097 x 2161 (n_px % 4 == 1: the tail next to the stride)

Every output buffer is filled with a poison value before the launch and has guard rails; afterwards EVERY pixel is accounted for.
The float64 filter checker is too slow for 16 M pixels, so the denoiser's tall frames repeat a block of PERIOD = 997 rows (not a
multiple of 16: every tile phase occurs) and a pixel goes one of two ways:
  checker   rows [0, PERIOD + S) and rows [yb - 48, H), yb the first row of tile 65 536 (both sides of the cap, the NaN / inf pixels
            placed in the second pass, the frame's end): against denoise_checker on a crop with S more rows at each cut
  periodic  rows [PERIOD + S, yb - 48): bit for bit equal to the row PERIOD above, which went one of the two ways itself.  The filter
            depends on position through addressing alone, and S = 2 (2^N - 1) + 1 + 2 rows (taps, variance prefilter, 5 x 5
            estimate) is its support, so these rows see the same values as their counterparts.
A skipped tile or pixel keeps the poison and fails whichever way it goes.  The temporal frame is not periodic (reprojection
depends on the pixel's ray): it is compared with temporal_checker over the whole frame, the filter in bands of rows."""
import numpy as np
import pytest

import denoise_checker as K
import display_checker as D
import scenes
import temporal_checker as T
from post_runners import SCENES, TOL, DeviceDisplay, bits_equal, check_display

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
PERIOD = 997
POISON = -12345.0
RAIL = 64  # floats on each side of a poisoned output
TALL = {"one_column": (1, 1048577), "edge_tiles": (17, 524300), "pixel_cap": (16, 1048592)}


def support(iterations):
    return 2 * (2 ** iterations - 1) + 1 + 2


def first_row_of_tile_65536(w):
    return 65536 // ((w + 15) // 16) * 16


@pytest.fixture(scope="module")
def dev_scene(hb):
    sc, cam_params = SCENES["rtweekend1"]()
    return hb.HipScene(sc, device=0), hb.camera_new(**cam_params)


def tall_inputs(w, h, seed, periodic=True):
    """a block of PERIOD rows repeated down the frame (or h fresh rows): normals scattered about +z and depths about 2, so that every
    weight of the filter is in play; one NaN in the block (so in every period); NaN / inf pixels in the rows of tile 65 536 and up"""
    rows = PERIOD if periodic else h
    rng = np.random.default_rng(seed)
    block = dict(color=rng.uniform(0.0, 2.0, (rows, w, 3)), albedo=rng.uniform(0.1, 1.0, (rows, w, 3)),
                 normal=np.array([0, 0, 1.0]) + 0.3 * rng.normal(size=(rows, w, 3)), depth=2.0 + 0.2 * rng.uniform(size=(rows, w)),
                 variance=rng.uniform(0, 0.2, (rows, w)))
    block["color"][PERIOD // 2, w // 2, 1] = np.nan
    reps = -(-h // rows)
    full = {k: np.ascontiguousarray(np.tile(v.astype(F32), (reps,) + (1,) * (v.ndim - 1))[:h]) for k, v in block.items()}
    yb = first_row_of_tile_65536(w)
    assert yb < h
    full["color"][yb, 0, 0] = np.nan
    full["color"][h - 1, w - 1, 2] = np.inf
    if h - yb > 4:
        full["color"][yb + 3, w // 2, 1] = -np.inf
        full["variance"][yb + 2, w - 1] = np.nan
    return full


class Poisoned:
    """a device output of n floats filled with POISON between two rails"""

    def __init__(self, torch, n):
        self.torch, self.n = torch, n
        self.t = torch.full((n + 2 * RAIL,), POISON, dtype=torch.float32, device=torch.device("cuda", 0))

    def ptr(self):
        return self.t.data_ptr() + 4 * RAIL

    def read(self, what):
        a = self.t.cpu().numpy()
        assert (a[:RAIL] == F32(POISON)).all() and (a[RAIL + self.n:] == F32(POISON)).all(), f"{what}: wrote outside the buffer"
        return a[RAIL:RAIL + self.n]


def run_denoise(torch, hb, gpu, inputs, what, **opts):
    """rt_denoise_device into a poisoned, railed output; the workspace is poisoned too (a plane pixel that is never written feeds
    the next iteration garbage)"""
    dev = torch.device("cuda", 0)
    h, w = inputs["color"].shape[:2]
    o = hb.denoise_opts(w, h, **opts)
    t = {k: torch.from_numpy(v).to(dev) for k, v in inputs.items()}
    ws = torch.full((hb.denoise_workspace_bytes(o),), 0xA5, dtype=torch.uint8, device=dev)
    out = Poisoned(torch, h * w * 3)
    torch.cuda.synchronize(dev)
    gpu.denoise_device({k: v.data_ptr() for k, v in t.items()}, ws.data_ptr(), out.ptr(), o, stream=0)
    torch.cuda.synchronize(dev)
    res = out.read(what).reshape(h, w, 3).copy()
    del t, ws, out
    torch.cuda.empty_cache()
    return res


def check_rows(out, inputs, a, b, lo, hi, what, **opts):
    """rows [a, b) of `out` against the checker on the crop [lo, hi) of the inputs"""
    crop = {k: v[lo:hi] for k, v in inputs.items()}
    ref = K.denoise(crop["color"], crop.get("albedo"), crop.get("normal"), crop.get("depth"), crop.get("variance"), **opts)[a - lo:b - lo]
    got, color = out[a:b], inputs["color"][a:b]
    valid = np.isfinite(color).all(axis=-1)
    if "variance" in inputs:
        valid &= np.isfinite(inputs["variance"][a:b])
    assert np.array_equal(got[~valid], color[~valid], equal_nan=True), f"{what}: invalid pixels pass through"
    err = K.relative_error(got[valid], ref[valid])
    assert err <= TOL, f"{what} rows {a}..{b}: relative error {err:.3e}"
    return int((~valid).sum())


def account_for_every_pixel(out, inputs, what, **opts):
    h, w = out.shape[:2]
    s = support(opts.get("iterations", 5))
    yb = first_row_of_tile_65536(w)
    head, tail = PERIOD + s, yb - 48
    assert head + PERIOD < tail and not (out == F32(POISON)).any(), f"{what}: poison left in the output"
    check_rows(out, inputs, 0, head, 0, head + s, f"{what} (head)", **opts)  # checker: the first period and the frame's top edge
    n_bad = check_rows(out, inputs, tail, h, tail - s, h, f"{what} (tiles 65 535 / 65 536 and up)", **opts)  # checker: across the cap
    assert n_bad >= 1  # the invalid pixels of the second pass
    bits = out.view(np.uint32)
    same = bits[head:tail] == bits[head - PERIOD:tail - PERIOD]  # periodic: every other row, against the row one period above
    assert same.all(), f"{what}: {int((~same).sum())} floats of rows {head}..{tail} differ from the row {PERIOD} above"


@pytest.mark.parametrize("shape", list(TALL))
def test_denoise_past_the_tile_and_pixel_caps(hb, dev_scene, shape):
    """with a given variance at 1 iteration (prepass<0>, the LAST kernel alone) and without one at 3 (prepass<1>, the variance
    kernel, two non-LAST iterations and the LAST one); pixel_cap is the frame whose per-pixel loops repeat"""
    import torch
    gpu, _ = dev_scene
    w, h = TALL[shape]
    assert ((w + 15) // 16) * ((h + 15) // 16) > 65536 and (shape != "pixel_cap" or w * h > 16777216)
    full = tall_inputs(w, h, seed=len(shape))
    out = run_denoise(torch, hb, gpu, full, f"{shape} variance", iterations=1)
    account_for_every_pixel(out, full, f"{shape} given variance, 1 iteration", iterations=1)
    no_var = {k: v for k, v in full.items() if k != "variance"}
    out = run_denoise(torch, hb, gpu, no_var, f"{shape} no variance", iterations=3)
    account_for_every_pixel(out, no_var, f"{shape} no variance, 3 iterations", iterations=3)


def test_render_denoised_past_the_pixel_cap(hb, dev_scene):
    """prepass<2> (the two halves of rt_render_denoised) at 16 x 1 048 592: the noisy mean it writes is checked on every pixel, and
    the clean frame equals rt_denoise of (noisy, AOVs, the halves' variance) byte for byte -- prepass<0> on the same frame shape,
    whose every pixel the test above accounts for"""
    gpu, cam = dev_scene
    w, h = TALL["pixel_cap"]
    spp = 2
    opts = abi.default_render_opts(w, h, spp, seed=5)
    dopts = hb.denoise_opts(0, 0, iterations=2)
    clean, noisy, _ = gpu.render_denoised(cam, opts, dopts)
    halves = []
    for begin in (0, 1):
        o = abi.default_render_opts(w, h, 1, seed=5)
        o.sample_begin = begin
        halves.append(gpu.render(cam, o)[0])
    assert noisy.tobytes() == ((halves[0] + halves[1]) * F32(0.5)).tobytes()
    aov = gpu.render_aov(cam, opts, channels=("albedo", "normal", "depth"))
    var = K.halves_variance(halves[0], halves[1], aov["albedo"])
    assert clean.tobytes() == gpu.denoise(noisy, aov, variance=var, iterations=2).tobytes()
    assert clean[-16:].tobytes() != noisy[-16:].tobytes()  # the last 256 pixels, the second pass of the per-pixel loop, were filtered


def test_temporal_past_the_pixel_cap(hb, dev_scene):
    """16 x 1 048 592, one iteration (so temporal_feedback also remodulates into out).  Frame 1 has no history: out equals rt_denoise
    byte for byte and the history planes are the checker's.  Frame 2 reads that history from the same camera (so that the pixels of the second pass keep theirs): motion, n,
    moments and guides bit for bit against temporal_checker.step over the whole frame, e_1 and out under TOL against the float64
    filter in bands of rows (the filter's support, 5 rows at one iteration, added at each cut).  All of out, motion and both
    histories start as poison."""
    import torch
    gpu, _ = dev_scene
    w, h = TALL["pixel_cap"]
    n = w * h
    dev = torch.device("cuda", 0)
    opts = hb.temporal_opts(w, h, iterations=1)
    p = dict(origin=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -5.0), vup=(0.0, 1.0, 0.0), fov=40.0, aspect_ratio=w / h, aperture=0.0, focus_dist=1.0)
    cams = [hb.camera_new(**p), hb.camera_new(**p)]  # static: the rows of the second pass must find their history
    hist = [Poisoned(torch, 12 * n) for _ in range(2)]
    ws = torch.full((hb.temporal_workspace_bytes(opts),), 0xA5, dtype=torch.uint8, device=dev)
    prev_hist = None
    for i, cam in enumerate(cams):
        f = {k: v for k, v in tall_inputs(w, h, seed=40 + i, periodic=False).items() if k != "variance"}
        f["depth"] = (f["depth"] * F32(2.5)).astype(F32)
        t = {k: torch.from_numpy(v).to(dev) for k, v in f.items()}
        out, motion = Poisoned(torch, 3 * n), Poisoned(torch, 2 * n)
        torch.cuda.synchronize(dev)
        gpu.denoise_temporal_device({k: v.data_ptr() for k, v in t.items()}, cam, cams[0] if i else None, hist[0].ptr() if i else 0,
                                    hist[i].ptr(), ws.data_ptr(), out.ptr(), opts, d_motion=motion.ptr(), stream=0)
        torch.cuda.synchronize(dev)
        got = out.read(f"frame {i} out").reshape(h, w, 3).copy()
        mv = motion.read(f"frame {i} motion").reshape(h, w, 2).copy()
        h_out = T.history_array(hist[i].read(f"frame {i} history"), h, w)
        del t, out, motion
        assert not (got == F32(POISON)).any() and not (h_out == F32(POISON)).any() and not (mv == F32(POISON)).any()
        st = T.step(f["color"], f["depth"], cam, cams[0] if i else None, prev_hist, albedo=f["albedo"], normal=f["normal"])
        assert bits_equal(mv, st["motion"]), f"frame {i}: motion"
        assert bits_equal(h_out[0, ..., 3], st["n"]) and bits_equal(h_out[1], st["history"][1]), f"frame {i}: n, n^ and z"
        assert bits_equal(h_out[2, ..., 0], st["m1"]) and bits_equal(h_out[2, ..., 1], st["m2"]) and not h_out[2, ..., 2:].any()
        ok = st["valid"]
        assert np.array_equal(got[~ok], f["color"][~ok], equal_nan=True) and (~ok).sum() >= 3
        if i == 0:
            assert np.isnan(mv).all()
            plain = run_denoise(torch, hb, gpu, f, "rt_denoise of frame 0", iterations=1)
            assert got.tobytes() == plain.tobytes()
        else:
            assert (st["n"] == 2).mean() > 0.1 and (st["n"] == 1).mean() > 0.001
            # the last 256 pixels are the second pass of temporal_resolve / temporal_feedback: unless some of them blend a history
            # in, e equals e0 there and a resolve that skipped them would go unseen
            last = st["n"][-16:] == 2
            assert last.sum() >= 16 and not bits_equal(st["e"][-16:][last], T.prepass(f["color"], f["albedo"])[1][-16:][last])
        band, s = 65536, support(1)
        for a in range(0, h, band):  # e_1 and out of every row against the float64 filter
            b, lo, hi = min(a + band, h), max(a - s, 0), min(a + band + s, h)
            crop = {k: (v[lo:hi] if isinstance(v, np.ndarray) and v.shape[:1] == (h,) else v) for k, v in st.items()}
            e1, ref = T.filtered(crop, f["color"][lo:hi], True, iterations=1)
            sel = (slice(a - lo, b - lo),)
            v = ok[a:b]
            err_e1 = K.relative_error(h_out[0, a:b][v][:, :3], e1[sel][v])
            err_out = K.relative_error(got[a:b][v], ref[sel][v])
            assert err_e1 <= TOL and err_out <= TOL, f"frame {i} rows {a}..{b}: e_1 {err_e1:.3e} out {err_out:.3e}"
        prev_hist = h_out
    del hist, ws
    torch.cuda.empty_cache()


@pytest.mark.parametrize("in_off,out_off,kw", [(0, 0, dict(pixel_format=D.RGBA8)),
                                               (0, 0, dict(pixel_format=D.RGB8, quantiser=D.ROUND, tonemap=D.REINHARD)),
                                               (1, 3, dict(pixel_format=D.BGRA8, quantiser=D.ROUND, transfer=D.GAMMA))])
def test_display_past_the_map_caps(hb, O, dev_scene, in_off, out_off, kw):
    """4097 x 2161 = 8 853 617 pixels: above the 8 388 608 of display_map<true> (aligned buffers; RGBA8 16-byte stores and RGB8
    12-byte stores) and the 4 194 304 of display_map<false> (offset buffers), n_px % 4 == 1.  Every byte, the histogram and the
    state against the checker; DeviceDisplay fills the output with 0x5A and checks its rails."""
    import torch
    gpu, _ = dev_scene
    w, h = 4097, 2161
    assert w * h > 8388608 and (w * h) % 4 != 0
    rng = np.random.default_rng(5)
    img = (rng.uniform(0.2, 1.0, (h, w, 3)).astype(F32) * np.exp2(rng.uniform(-6.0, 4.0, (h, w, 1))).astype(F32))
    img[h - 1, w - 1] = (np.nan, 1.0, 1.0)
    run = DeviceDisplay(torch, hb, gpu, w, h, in_off, out_off, **kw)
    check_display(O, run, img, (F32(0.5), 2, F32(0)), f"4097x2161 offsets {in_off},{out_off}", **kw)
    del run
    torch.cuda.empty_cache()
