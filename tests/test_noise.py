"""The noise estimates (rt_render_noise, rt_noise_tiles, rt_render_converged, rt_render_denoised_split) without a GPU: the C-ABI
boundary on a host-only scene -- structs, defaults, the split rule and the status code of every check -- then the numpy checker
(tests/noise_checker.py) held to hand-computed cases, and one statistical check that the estimator estimates what it claims."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import noise_checker as N
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32


# ---- the C-ABI boundary ----
def test_struct_sizes_against_a_compiled_sizeof(tmp_path):
    names = {"rt_noise_opts": abi.NoiseOpts, "rt_noise_summary": abi.NoiseSummary, "rt_noise_buffers": abi.NoiseBuffers,
             "rt_noise_result": abi.NoiseResult}
    src = '#include <stdio.h>\n#include "rt_hip.h"\nint main(void){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "return 0;}"
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    sizes = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in names.items():
        assert int(sizes[n]) == C.sizeof(cls) == abi.EXPECTED_SIZES[n][1], (n, sizes[n], C.sizeof(cls))
        assert abi.EXPECTED_SIZES[n][0] is cls


def test_defaults(hb):
    lib = hb.lib()
    o = abi.NoiseOpts()
    o.luminance_floor, o.threshold = 7.0, 7.0
    o.reserved[3] = 9
    assert lib.rt_noise_opts_default(C.byref(o)) == abi.RT_OK
    assert (F32(o.luminance_floor), F32(o.threshold)) == (F32(0.01), F32(0.05)) and list(o.reserved) == [0] * 6
    assert bytes(abi.default_noise_opts()) == bytes(o) == bytes(hb.noise_opts())
    assert lib.rt_noise_opts_default(None) == abi.RT_ERR_INVALID_ARGUMENT
    n = hb.noise_opts(threshold=0.5)
    assert (n.threshold, F32(n.luminance_floor)) == (0.5, F32(0.01))
    with pytest.raises(ValueError):
        hb.noise_opts(floor=1.0)


def _arrays(w, h):
    keep = {"mean": np.zeros(3 * w * h, F32), "variance": np.zeros(w * h, F32), "lum_mean": np.zeros(w * h, F32),
            "tile_error": np.zeros(((w + 7) // 8) * ((h + 7) // 8), F32), "albedo": np.zeros(3 * w * h, F32)}
    summary = abi.NoiseSummary()
    b = abi.NoiseBuffers()
    for name in ("mean", "variance", "lum_mean", "tile_error"):
        setattr(b, name, keep[name].ctypes.data_as(C.POINTER(C.c_float)))
    b.summary = C.pointer(summary)
    keep["summary"] = summary
    return b, keep


def _at(array, index):
    return C.cast(C.c_void_p(array.ctypes.data + 4 * index), C.POINTER(C.c_float))


def _opts(w, h, spp, split):
    o = abi.default_render_opts(w, h, spp)
    o.sample_split = split
    return o


@pytest.fixture(scope="module")
def host_only(hb):
    ls = scenes.load_ssml("rtweekend1")
    return hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE), hb.camera_new(**ls.camera_params)


def test_render_noise_status_codes_and_the_split_rule_without_a_device(hb, host_only):
    s, cam = host_only
    lib = hb.lib()
    w, h = 16, 9
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    INVALID, UNSUPPORTED, NO_DEVICE = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE

    def call(opts, nopts, bufs, device, albedo=None, scene=s._h, camera=cam):
        if device:
            return lib.rt_render_noise_device(scene, ref(camera), ref(opts), ref(nopts), albedo, ref(bufs), None, C.c_void_p(0))
        return lib.rt_render_noise(scene, ref(camera), ref(opts), ref(nopts), albedo, ref(bufs), None)

    no = abi.default_noise_opts()
    for device in (False, True):
        full, keep = _arrays(w, h)
        ok = _opts(w, h, 8, 2)
        assert call(ok, no, full, device) == NO_DEVICE
        assert call(ok, no, full, device, albedo=_at(keep["albedo"], 0)) == NO_DEVICE
        only_mean = abi.NoiseBuffers()
        only_mean.mean = full.mean
        assert call(ok, no, only_mean, device) == NO_DEVICE  # any field but the mean may be NULL
        no_mean, _ = _arrays(w, h)
        no_mean.mean = None
        assert call(ok, no, no_mean, device) == INVALID
        for args in ((None, no, full), (ok, None, full), (ok, no, None)):
            assert call(*args, device) == INVALID
        assert call(ok, no, full, device, scene=None) == INVALID
        assert call(ok, no, full, device, camera=None) == INVALID
        # the split rule
        for spp, split in ((8, 2), (8, 4), (8, 8), (64, 64), (6, 3), (1024, 0), (32, 0), (100, 0), (102, 0)):  # (100: 8 halved to 4)
            assert call(_opts(w, h, spp, split), no, full, device) == NO_DEVICE, (spp, split)
        for spp, split in ((8, 3), (8, 1), (7, 0), (1, 0), (33, 0), (8, 0), (8, 16),  # (8, 0): chunks of 16 passes leave no split
                            (128, 128), (130, 65), (8, 5), (0, 2), (1 << 32, 2)):
            assert call(_opts(w, h, spp, split), no, full, device) == INVALID, (spp, split)
        # options
        for bad in (dict(luminance_floor=0.0), dict(luminance_floor=-0.01), dict(luminance_floor=np.inf), dict(luminance_floor=np.nan),
                    dict(threshold=-1e-30), dict(threshold=np.inf), dict(threshold=np.nan)):
            assert call(ok, abi.default_noise_opts(**bad), full, device) == INVALID, bad
        assert call(ok, abi.default_noise_opts(threshold=0.0), full, device) == NO_DEVICE
        assert call(ok, abi.default_noise_opts(luminance_floor=1e-30), full, device) == NO_DEVICE
        for word in range(6):
            n = abi.default_noise_opts()
            n.reserved[word] = 1
            assert call(ok, n, full, device) == INVALID, word
        # overlap: an output on the last value of another output, of the albedo; just behind it is fine
        n_px = w * h
        b, keep = _arrays(w, h)
        b.variance = _at(keep["mean"], 3 * n_px - 1)
        assert call(ok, no, b, device) == INVALID
        b, keep = _arrays(w, h)
        b.lum_mean = _at(keep["variance"], n_px - 1)
        assert call(ok, no, b, device) == INVALID
        b, keep = _arrays(w, h)
        b.tile_error = _at(keep["lum_mean"], n_px - 1)
        assert call(ok, no, b, device) == INVALID
        b, keep = _arrays(w, h)
        b.summary = C.cast(C.c_void_p(keep["tile_error"].ctypes.data + 4 * (len(keep["tile_error"]) - 1)), C.POINTER(abi.NoiseSummary))
        assert call(ok, no, b, device) == INVALID
        b, keep = _arrays(w, h)
        assert call(ok, no, b, device, albedo=_at(keep["mean"], 3 * n_px - 1)) == INVALID
        big = np.zeros(4 * n_px, F32)
        b, keep = _arrays(w, h)
        b.mean, b.variance = _at(big, 0), _at(big, 3 * n_px)
        assert call(ok, no, b, device) == NO_DEVICE
        # the frame
        o = _opts(w, h, 8, 2)
        o.output_layout = abi.RT_LAYOUT_SHARD
        assert call(o, no, full, device) == UNSUPPORTED
        o = _opts(w, h, 8, 2)
        o.shard_count = 2
        assert call(o, no, full, device) == UNSUPPORTED
        assert call(_opts(1, h, 8, 2), no, full, device) == INVALID
        assert call(_opts(w, 1, 8, 2), no, full, device) == INVALID
        o = _opts(w, h, 8, 2)
        o.render_method = 7
        assert call(o, no, full, device) == INVALID
    # the Python binding
    with pytest.raises(hb.RtHipError) as e:
        s.render_noise(cam, _opts(w, h, 8, 2))
    assert e.value.code == NO_DEVICE
    with pytest.raises(hb.RtHipError) as e:
        s.render_noise(cam, _opts(w, h, 8, 3))
    assert e.value.code == INVALID
    with pytest.raises(hb.RtHipError) as e:
        s.render_noise(cam, _opts(w, h, 7, 0))
    assert e.value.code == INVALID
    with pytest.raises(hb.RtHipError) as e:
        s.render_noise(cam, _opts(w, h, 8, 1))
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        s.render_noise(cam, _opts(w, h, 8, 2), channels=("stats",))


def test_noise_tiles_status_codes_without_a_device(hb, host_only):
    s, _ = host_only
    lib = hb.lib()
    INVALID, NO_DEVICE = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_NO_DEVICE
    w, h = 13, 11
    lum, var, tiles = np.zeros(w * h, F32), np.zeros(w * h, F32), np.zeros(4, F32)
    summary = abi.NoiseSummary()
    no = abi.default_noise_opts()

    def call(device, lum_p=_at(lum, 0), var_p=_at(var, 0), width=w, height=h, nopts=no, tile_p=_at(tiles, 0), sum_p=C.pointer(summary),
             scene=s._h):
        f = lib.rt_noise_tiles_device if device else lib.rt_noise_tiles
        args = (scene, lum_p, var_p, C.c_uint32(width), C.c_uint32(height), C.byref(nopts) if nopts is not None else None, tile_p, sum_p)
        return f(*args, C.c_void_p(0)) if device else f(*args)

    for device in (False, True):
        assert call(device) == NO_DEVICE
        assert call(device, tile_p=None) == NO_DEVICE and call(device, sum_p=None) == NO_DEVICE
        assert call(device, width=1, height=1) == NO_DEVICE  # a frame of one pixel is a frame
        assert call(device, tile_p=None, sum_p=None) == INVALID
        assert call(device, lum_p=None) == INVALID and call(device, var_p=None) == INVALID
        assert call(device, nopts=None) == INVALID and call(device, scene=None) == INVALID
        assert call(device, width=0) == INVALID and call(device, height=0) == INVALID
        assert call(device, nopts=abi.default_noise_opts(luminance_floor=0.0)) == INVALID
        assert call(device, nopts=abi.default_noise_opts(threshold=-1.0)) == INVALID
        assert call(device, tile_p=_at(var, w * h - 1)) == INVALID  # written over a plane read
        assert call(device, sum_p=C.cast(C.c_void_p(tiles.ctypes.data + 12), C.POINTER(abi.NoiseSummary))) == INVALID
        assert call(device, width=1 << 16, height=(1 << 15) + 1) == abi.RT_ERR_UNSUPPORTED


def test_converged_and_denoised_split_status_codes_without_a_device(hb, host_only):
    s, cam = host_only
    lib = hb.lib()
    INVALID, UNSUPPORTED, NO_DEVICE = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE
    w, h = 16, 9
    n_px = w * h
    mean, var, tiles = np.zeros(3 * n_px, F32), np.zeros(n_px, F32), np.zeros(4, F32)
    res = abi.NoiseResult()
    no = abi.default_noise_opts()

    def conv(opts, batch, min_batches=1, max_passes=64, nopts=no, mean_p=_at(mean, 0), var_p=_at(var, 0), tile_p=_at(tiles, 0), result=res):
        return lib.rt_render_converged(s._h, C.byref(cam), C.byref(opts), C.byref(nopts) if nopts is not None else None, C.c_uint64(batch),
                                       C.c_uint32(min_batches), C.c_uint64(max_passes), mean_p, var_p, tile_p,
                                       C.byref(result) if result is not None else None)

    ok = _opts(w, h, 999, 2)  # samples_per_pixel is ignored: the rule applies to the batch
    assert conv(ok, 8) == NO_DEVICE
    assert conv(ok, 8, var_p=None, tile_p=None) == NO_DEVICE
    assert conv(ok, 8, max_passes=8) == NO_DEVICE
    assert conv(ok, 0) == INVALID  # batch = 0
    assert conv(ok, 8, max_passes=7) == INVALID  # max_passes < batch
    assert conv(ok, 7) == INVALID and conv(_opts(w, h, 8, 0), 7) == INVALID and conv(_opts(w, h, 8, 3), 8) == INVALID
    assert conv(_opts(w, h, 8, 1), 8) == INVALID
    assert conv(_opts(w, h, 7, 0), 32) == NO_DEVICE
    assert conv(ok, 8, mean_p=None) == INVALID and conv(ok, 8, result=None) == INVALID and conv(ok, 8, nopts=None) == INVALID
    assert conv(ok, 8, nopts=abi.default_noise_opts(threshold=np.nan)) == INVALID
    assert conv(ok, 8, var_p=_at(mean, 3 * n_px - 1)) == INVALID
    assert conv(ok, 8, tile_p=_at(var, n_px - 1)) == INVALID
    o = _opts(w, h, 8, 2)
    o.shard_count = 2
    assert conv(o, 8) == UNSUPPORTED

    clean, noisy = np.zeros(3 * n_px, F32), np.zeros(3 * n_px, F32)
    d = abi.default_denoise_opts()

    def den(opts, dopts=d, clean_p=_at(clean, 0), noisy_p=_at(noisy, 0), var_p=_at(var, 0)):
        return lib.rt_render_denoised_split(s._h, C.byref(cam), C.byref(opts), C.byref(dopts) if dopts is not None else None, clean_p, noisy_p,
                                            var_p, None)

    ok = _opts(w, h, 8, 4)
    assert den(ok) == NO_DEVICE and den(ok, noisy_p=None, var_p=None) == NO_DEVICE
    assert den(ok, clean_p=None) == INVALID and den(ok, dopts=None) == INVALID
    assert den(_opts(w, h, 8, 3)) == INVALID and den(_opts(w, h, 7, 0)) == INVALID and den(_opts(w, h, 8, 1)) == INVALID
    assert den(ok, dopts=abi.default_denoise_opts(iterations=11)) == INVALID
    assert den(ok, noisy_p=_at(clean, 3 * n_px - 1)) == INVALID
    assert den(ok, var_p=_at(noisy, 3 * n_px - 1)) == INVALID
    o = _opts(w, h, 8, 4)
    o.output_layout = abi.RT_LAYOUT_SHARD
    assert den(o) == UNSUPPORTED


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() { rt_hip::NoiseOptions n; n.threshold = 0.1f;\n'
           'rt_hip::NoiseEstimate (*f)(const rt_hip::RenderOptions &, const rt_hip::SimpleCamera &, const rt_hip::Bvh &, uint32_t, '
           'const rt_hip::NoiseOptions &, uint64_t, uint64_t) = &rt_hip::render_noise; (void)f;\n'
           'rt_hip::ConvergedFrame (*g)(const rt_hip::RenderOptions &, const rt_hip::SimpleCamera &, const rt_hip::Bvh &, uint32_t, '
           'uint64_t, uint32_t, uint64_t, const rt_hip::NoiseOptions &, uint64_t) = &rt_hip::render_converged; (void)g;\n'
           'rt_hip::NoiseEstimate e; return (int)(e.mean.size() + e.summary.n_tiles + n.luminance_floor); }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)


# ---- the checker against hand-computed cases ----
def _ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_two_chunks_give_the_squared_half_difference():
    """S = 2: lbar = (l0 + l1) / 2, both deviations are (l0 - l1) / 2 up to rounding, var = 2 ((l0 - l1) / 2)^2 / 2 =
    (l0 - l1)^2 / 4 -- rt_render_denoised's formula.  The two differ by the roundings of lbar and of the two deviations: within
    4 ulp, or 1e-12 absolute where the difference of the chunks itself cancels to nearly nothing."""
    rng = np.random.default_rng(5)
    sums = rng.uniform(0.0, 8.0, (2, 6, 5, 3)).astype(F32)
    sums[1, 0, 0] = sums[0, 0, 0]  # equal chunks: variance exactly 0
    sums[1, 0, 1] = np.nextafter(sums[0, 0, 1], F32(9))
    albedo = rng.uniform(0.0, 1.0, (6, 5, 3)).astype(F32)
    albedo[1, 1] = 0.0  # floored to 1e-3
    for alb in (None, albedo):
        mean, lbar, var = N.estimate(sums, 8, alb)
        d = np.fmax(alb, F32(1e-3)) if alb is not None else F32(1.0)
        l0, l1 = N.lum(sums[0] / F32(4) / d), N.lum(sums[1] / F32(4) / d)
        expected = (l0 - l1) * (l0 - l1) / F32(4)
        close = (_ulps(var, expected) <= 4) | (np.abs(var.astype(np.float64) - expected) <= 1e-12)
        assert close.all(), (var[~close], expected[~close])
        assert var[0, 0] == 0.0 and mean.tobytes() == ((sums[0] + sums[1]) / F32(8)).tobytes()
        assert var.dtype == lbar.dtype == mean.dtype == F32


def test_a_constant_frame_has_no_variance_and_no_error():
    passes = np.broadcast_to(F32(0.375), (8, 11, 13, 3)).copy()
    for split in (2, 4, 8):
        mean, lbar, var = N.estimate(N.chunk_sums(passes, split), 8)
        assert (mean == F32(0.375)).all() and (var == 0.0).all() and not np.signbit(var).any()
        err, summary = N.tiles(lbar, var)
        assert (err == 0.0).all() and summary == {"max_tile_error": F32(0.0), "tiles_above": 0, "n_tiles": 4}
    m, l, v = N.accumulate([(mean, lbar, var)] * 3)
    assert (m == F32(0.375)).all() and (v == 0.0).all() and l.tobytes() == ((lbar + lbar + lbar) / F32(3)).tobytes()


def test_one_batch_accumulates_to_itself():
    rng = np.random.default_rng(6)
    passes = rng.uniform(0.0, 2.0, (8, 4, 4, 3)).astype(F32)
    passes[3, 1, 1] = np.inf
    passes[2, 2, 2] = np.nan
    one = N.estimate(N.chunk_sums(passes, 4), 8)
    for got, ref in zip(N.accumulate([one]), one):
        assert got.tobytes() == ref.tobytes()  # x / 1.0f = x, NaN and inf included
    assert np.isnan(one[2][1, 1]) and np.isnan(one[2][2, 2])  # inf - inf, and the NaN


def test_absent_slots_and_edge_tiles_counted_by_hand_on_13_by_11():
    """tiles (0, 0) whole, (1, 0) 5 x 8, (0, 1) 8 x 3, (1, 1) 5 x 3; r = sqrt(v) / (|l| + floor) chosen exactly representable"""
    w, h, floor = 13, 11, 0.25
    lum = np.full((h, w), 0.75, F32)  # |l| + floor = 1
    var = np.zeros((h, w), F32)
    var[0:8, 0:8] = 0.25    # r = 0.5 on 64 pixels  -> 0.5
    var[0:8, 8:13] = 4.0    # r = 2 on 40 pixels    -> 80 / 40 = 2
    var[8:11, 0:8] = 1.0    # r = 1 on 24 pixels    -> 1
    var[8:11, 8:13] = 0.0625  # r = 0.25 on 15 pixels -> 3.75 / 15 = 0.25
    lum[9, 9] = -0.75       # fabsf: the same r
    slots, count = N.tile_slots(lum, var, floor)
    assert count.tolist() == [[64, 40], [24, 15]]
    assert (slots[0, 1].reshape(8, 8)[:, 5:] == 0).all() and (slots[0, 1].reshape(8, 8)[:, :5] == 2).all()
    assert (slots[1, 1].reshape(8, 8)[3:, :] == 0).all() and (slots[1, 1].reshape(8, 8)[:3, 5:] == 0).all()
    assert int((slots[1, 1] != 0).sum()) == 15 and not np.signbit(slots).any()
    err, summary = N.tiles(lum, var, floor, threshold=1.0)
    assert err.tolist() == [[0.5, 2.0], [1.0, 0.25]]
    assert summary == {"max_tile_error": F32(2.0), "tiles_above": 1, "n_tiles": 4}  # strictly above 1: the tile at exactly 1 is not
    # one non-finite pixel makes its tile +inf and leaves the others alone
    for bad_var, bad_lum in ((np.nan, 0.75), (np.inf, 0.75), (-1.0, 0.75), (1.0, np.nan)):
        v2, l2 = var.copy(), lum.copy()
        v2[10, 12], l2[10, 12] = bad_var, bad_lum
        e2, s2 = N.tiles(l2, v2, floor, threshold=1.0)
        assert e2[1, 1] == np.inf and e2.reshape(-1)[:3].tolist() == [0.5, 2.0, 1.0], (bad_var, bad_lum)
        assert s2 == {"max_tile_error": F32(np.inf), "tiles_above": 2, "n_tiles": 4}


def test_the_butterfly_is_a_tree_not_a_running_sum():
    """values a running sum would round differently: the tree adds neighbours first"""
    h = w = 8
    var = np.ones((h, w), F32)
    var[0, 0] = F32(2.0 ** 48)  # r = 2^24: absorbs 1 when added alone, not 2
    lum = np.full((h, w), 0.5, F32)
    err, _ = N.tiles(lum, var, 0.5)
    tree = np.sqrt(var).reshape(-1)
    while len(tree) > 1:
        tree = tree[0::2] + tree[1::2]
    running = F32(0)
    for x in np.sqrt(var).reshape(-1):
        running = F32(running + x)
    assert err[0, 0] == tree[0] / F32(64) and tree[0] != running


# ---- the estimator estimates what it claims ----
def test_the_mean_variance_estimate_is_the_variance_of_lum_mean(O):
    """Over seeds i = 1 .. N a 4 x 4 frame is rendered at spp = 8, S = 4.  Per pixel, `variance` claims to be an unbiased estimate
    of Var(lum_mean) (the sample variance of S independent, identically distributed chunk values divided by S), so with
    A_i = sum over pixels of variance_i and B = sum over pixels of the empirical variance of lum_mean over the seeds, E[mean A] =
    E[B] and the ratio mean(A) / B estimates 1.
    The band comes from the ratio's own sampling error.  mean(A) has standard error sd(A_i) / sqrt(N).  B = sum_i D_i / (N - 1)
    with D_i = sum over pixels of (lum_mean_i - mean over seeds)^2, a mean of N nearly independent terms: standard error
    sd(D_i) sqrt(N) / (N - 1).  To first order the relative error of the ratio is the root of the two relative errors squared
    (the delta method; the covariance of A and B is positive -- a seed with a wild sample raises both -- so this over-states it).
    Accepted: |ratio - 1| <= 4 of those, a 6e-5 event for a normal error.  N = 384 is chosen so that the band is narrow enough to
    tell the estimator from its plausible mistakes: dividing by S * S instead of S * (S - 1) gives 0.75, by (S - 1) alone 4,
    forgetting the chunk length nothing (l_c are means already): the test demands a band within +-0.2 before it asserts."""
    n_seeds, w, h, spp, split = 384, 4, 4, 8, 4
    cpu = O.Scene(scenes.all_materials())
    cam = O.camera_new(**scenes.ALL_MATERIALS_CAMERA)
    a, lums = np.zeros(n_seeds), np.zeros((n_seeds, h, w))
    for i in range(n_seeds):
        o = abi.default_render_opts(w, h, spp, method=abi.RT_METHOD_MIS, seed=1000 + i)
        _, lbar, var = N.render_estimate(cpu, cam, o, split)
        a[i], lums[i] = var.astype(np.float64).sum(), lbar
    d = ((lums - lums.mean(axis=0)) ** 2).sum(axis=(1, 2))
    b = d.sum() / (n_seeds - 1)
    ratio = a.mean() / b
    rel_a = a.std(ddof=1) / np.sqrt(n_seeds) / a.mean()
    rel_b = d.std(ddof=1) * np.sqrt(n_seeds) / (n_seeds - 1) / b
    band = 4.0 * np.hypot(rel_a, rel_b)
    print(f"mean variance {a.mean():.4e} empirical {b:.4e} ratio {ratio:.4f} band +-{band:.4f} (relative errors {rel_a:.4f}, {rel_b:.4f})")
    assert a.mean() > 0 and band < 0.2, band
    assert abs(ratio - 1.0) <= band, (ratio, band)
