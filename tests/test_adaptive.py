"""rt_render_tiles and rt_noise_select_tiles without a GPU: every status code of the four entry points on a host-only scene, in
the order include/rt_hip.h states (argument errors, then RT_ERR_UNSUPPORTED, then RT_ERR_NO_DEVICE), the list checks of the host
entry, and the split rule."""
import ctypes as C

import numpy as np

import scenes

abi = scenes.abi
F32 = np.float32
OK, INVALID, UNSUPPORTED, NO_DEVICE = abi.RT_OK, abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE
W, H = 24, 20  # 3 x 3 tiles


def _scene(hb):
    ls = scenes.load_ssml("rtweekend1")
    return hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE), hb.camera_new(**ls.camera_params)


def test_render_tiles_status_codes_without_a_device(hb):
    s, cam = _scene(hb)
    lib = hb.lib()
    frame = np.full((H, W, 3), 7.0, F32)
    sums = np.full((4, 9, 8, 8, 3), 7.0, F32)
    tiles = np.arange(9, dtype=np.uint32)
    rays = C.c_uint64(99)

    def call(device, *, scene=s._h, camera=cam, tiles=tiles, n=None, out=frame, sums=None, no_opts=False, **fields):
        o = abi.default_render_opts(W, H, 8, method=abi.RT_METHOD_MIS, seed=1)
        for k, v in fields.items():
            setattr(o, k, v)
        args = (scene, C.byref(camera) if camera is not None else None, None if no_opts else C.byref(o),
                C.c_void_p(tiles.ctypes.data) if tiles is not None else None, C.c_uint32(len(tiles) if n is None else n),
                C.c_void_p(out.ctypes.data) if out is not None else None, C.c_void_p(sums.ctypes.data) if sums is not None else None, C.byref(rays))
        return lib.rt_render_tiles_device(*args, C.c_void_p(0)) if device else lib.rt_render_tiles(*args)

    for device in (False, True):
        assert call(device) == NO_DEVICE
        for good in (dict(sample_split=0), dict(sample_split=1), dict(sample_split=8), dict(sample_split=3), dict(render_method=abi.RT_METHOD_NAIVE),
                     dict(tile_width=4, tile_height=16), dict(sample_begin=(1 << 64) - 1), dict(samples_per_pixel=(1 << 32) - 1)):
            assert call(device, **good) == NO_DEVICE, good
        assert call(device, sums=sums, sample_split=4) == NO_DEVICE
        assert call(device, n=0) == NO_DEVICE
        assert call(device, n=0, tiles=None) == NO_DEVICE
        # a host-only scene reports bad arguments as such
        assert call(device, scene=None) == INVALID
        assert call(device, camera=None) == INVALID
        assert call(device, no_opts=True) == INVALID
        assert call(device, out=None) == INVALID
        assert call(device, tiles=None, n=3) == INVALID
        for bad in (dict(width=1), dict(height=1), dict(samples_per_pixel=0), dict(samples_per_pixel=1 << 32), dict(render_method=2),
                    dict(render_method=-1), dict(output_layout=2), dict(shard_count=0), dict(shard_count=2, shard_index=2),
                    dict(sample_split=9)):  # (a split above the passes, as rt_render refuses it)
            assert call(device, **bad) == INVALID, bad
        assert call(device, n=10) == (NO_DEVICE if device else INVALID)  # more tiles than the frame has: the host entry's check alone
        # the chunk buffer must not overlap the frame (it is read only when S > 1)
        assert call(device, sums=frame, sample_split=2) == INVALID
        assert call(device, sums=frame, sample_split=1) == NO_DEVICE
        # unsupported comes after the argument errors and before the device
        for bad in (dict(output_layout=abi.RT_LAYOUT_SHARD), dict(shard_count=2), dict(width=1 << 16, height=1 << 15)):
            assert call(device, n=1, **bad) == UNSUPPORTED, bad
        assert call(device, n=1, output_layout=abi.RT_LAYOUT_SHARD, samples_per_pixel=0) == INVALID
    # the host entry checks the list: distinct, below the tile count -- ahead of the device
    for bad in ([0, 9], [3, 3], [8, 1, 8], [0xFFFFFFFF]):
        assert call(False, tiles=np.array(bad, np.uint32)) == INVALID, bad
        assert call(True, tiles=np.array(bad, np.uint32)) == NO_DEVICE, bad  # (the device entry cannot read a device list)
    assert (frame == 7.0).all() and (sums == 7.0).all() and rays.value == 99


def test_select_tiles_status_codes_without_a_device(hb):
    s, _ = _scene(hb)
    lib = hb.lib()
    err = np.zeros(9, F32)
    tiles = np.full(9, 5, np.uint32)
    count = C.c_uint32(77)

    def call(device, *, scene=s._h, err=err, w=W, h=H, threshold=0.05, tiles=tiles, count=count):
        args = (scene, C.c_void_p(err.ctypes.data) if err is not None else None, C.c_uint32(w), C.c_uint32(h), C.c_float(threshold),
                C.c_void_p(tiles.ctypes.data) if tiles is not None else None, C.byref(count) if count is not None else None)
        return lib.rt_noise_select_tiles_device(*args, C.c_void_p(0)) if device else lib.rt_noise_select_tiles(*args)

    for device in (False, True):
        assert call(device) == NO_DEVICE
        for threshold in (0.0, -1.0, np.inf, -np.inf):
            assert call(device, threshold=threshold) == NO_DEVICE
        assert call(device, w=1, h=1) == NO_DEVICE
        assert call(device, scene=None) == INVALID
        assert call(device, err=None) == INVALID
        assert call(device, tiles=None) == INVALID
        assert call(device, count=None) == INVALID
        assert call(device, threshold=np.nan) == INVALID
        assert call(device, w=0) == INVALID
        assert call(device, h=0) == INVALID
        assert call(device, tiles=err.view(np.uint32)) == INVALID  # the list overlaps the plane
        assert call(device, w=1 << 31, h=2) == UNSUPPORTED
    assert (tiles == 5).all() and count.value == 77


def test_bindings_refuse_bad_frames(hb):
    import pytest
    s, cam = _scene(hb)
    o = abi.default_render_opts(W, H, 4, seed=1)
    for frame in (np.zeros((H, W, 3), np.float64), np.zeros((H, W), F32), np.zeros((W, H, 3), F32)):
        with pytest.raises(ValueError):
            s.render_tiles(cam, o, [0], frame)
    with pytest.raises(ValueError):
        s.noise_select_tiles(np.zeros(9, F32), 0.5)


# ---- rt_render_adaptive: the struct, the status codes, and the numpy checker against hand cases ----
def test_struct_sizes_against_a_compiled_sizeof(tmp_path):
    import os
    import subprocess
    names = {"rt_adaptive_result": abi.AdaptiveResult, "rt_noise_result": abi.NoiseResult, "rt_noise_opts": abi.NoiseOpts}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "".join(
        f'printf("off_{f} %zu\\n", offsetof(rt_adaptive_result, {f}));' for f in ("pixel_passes", "rays_shot", "batches", "converged", "summary")) + "return 0;}"
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(scenes.ROOT, "include"), c, "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in names.items():
        assert int(got[n]) == C.sizeof(cls) == abi.EXPECTED_SIZES[n][1] and abi.EXPECTED_SIZES[n][0] is cls, n
    for f in ("pixel_passes", "rays_shot", "batches", "converged", "summary"):
        assert int(got["off_" + f]) == getattr(abi.AdaptiveResult, f).offset, f


def test_render_adaptive_status_codes_without_a_device(hb):
    s, cam = _scene(hb)
    lib = hb.lib()
    px, nt = W * H, 9
    mean, var, tiles, passes = np.full(3 * px, 7.0, F32), np.full(px, 7.0, F32), np.full(nt, 7.0, F32), np.full(px, 7, np.uint32)
    alb = np.full(3 * px, 0.5, F32)
    res = abi.AdaptiveResult()
    res.batches = 55

    def call(*, scene=s._h, camera=cam, nopts=None, no_opts=False, no_nopts=False, albedo=None, batch=4, min_batches=1, max_passes=16,
             mean=mean, var=var, tiles=tiles, passes=passes, result=res, **fields):
        o = abi.default_render_opts(W, H, 1, method=abi.RT_METHOD_MIS, seed=1)
        o.sample_split = 2
        for k, v in fields.items():
            setattr(o, k, v)
        n = hb.noise_opts() if nopts is None else nopts
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        return lib.rt_render_adaptive(scene, C.byref(camera) if camera is not None else None, None if no_opts else C.byref(o),
                                      None if no_nopts else C.byref(n), ptr(albedo), C.c_uint64(batch), C.c_uint32(min_batches),
                                      C.c_uint64(max_passes), ptr(mean), ptr(var), ptr(tiles), ptr(passes),
                                      C.byref(result) if result is not None else None)

    assert call() == NO_DEVICE
    for good in (dict(albedo=alb), dict(var=None), dict(tiles=None), dict(passes=None), dict(min_batches=0), dict(sample_split=4),
                 dict(sample_split=0, batch=64, max_passes=64), dict(batch=4, max_passes=4 * ((1 << 24) - 1)),
                 dict(nopts=hb.noise_opts(threshold=0.0))):
        assert call(**good) == NO_DEVICE, good
    for bad in (dict(scene=None), dict(camera=None), dict(no_opts=True), dict(no_nopts=True), dict(mean=None), dict(result=None),
                dict(batch=0), dict(max_passes=3), dict(width=1), dict(render_method=2),
                dict(sample_split=3), dict(sample_split=1), dict(sample_split=8), dict(sample_split=0, batch=3, max_passes=3),  # the split rule on `batch`
                dict(nopts=hb.noise_opts(threshold=float("nan"))), dict(nopts=hb.noise_opts(luminance_floor=0.0)),
                dict(var=mean[:px]), dict(tiles=var[:nt]), dict(passes=mean[:px].view(np.uint32)), dict(albedo=mean)):  # overlapping buffers
        assert call(**bad) == INVALID, bad
    for bad in (dict(output_layout=abi.RT_LAYOUT_SHARD), dict(shard_count=2), dict(batch=2, max_passes=2 << 24)):
        assert call(**bad) == UNSUPPORTED, bad
    assert call(batch=2, max_passes=(2 << 24) - 1) == NO_DEVICE
    assert (mean == 7.0).all() and (passes == 7).all() and res.batches == 55


def _hand(values_per_batch, w, h, batch=2, split=2):
    """batch_passes for the checker: window b holds per-pixel values values_per_batch[b] (h, w) with a +-delta pattern over its
    passes, so that the chunk sums differ and the variance is known"""
    def batch_passes(b):
        v, d = values_per_batch[b]
        p = np.zeros((batch, h, w, 3), F32)
        for i in range(batch):
            p[i] = (np.asarray(v, F32) + (F32(d) if i % 2 == 0 else -F32(d)))[..., None]
        return p
    return batch_passes


def test_checker_a_stopped_tile_keeps_its_bytes_while_its_neighbour_moves():
    import adaptive_checker as A
    w, h = 16, 8  # two tiles
    noisy = np.zeros((h, w), F32)
    noisy[:, 8:] = 1.0  # delta only in the right tile
    batches = [(np.ones((h, w), F32), 0.5 * noisy), (np.ones((h, w), F32) * 2, 0.5 * noisy), (np.ones((h, w), F32) * 3, 0.25 * noisy),
               (np.ones((h, w), F32) * 5, 0.25 * noisy)]
    r2 = A.adaptive(_hand(batches, w, h), w, h, 2, 2, 2, 4, threshold=0.05)  # (the right tile's error after batch 4 is 0.072)
    r4 = A.adaptive(_hand(batches, w, h), w, h, 2, 2, 2, 8, threshold=0.05)
    assert r2["batches"] == 2 and r4["batches"] == 4 and not r4["converged"]
    assert [a.tolist() for a in r4["active"]] == [[1]] * 4 and r4["rendered"][2].tolist() == [1]
    for k in ("mean", "variance", "lum_mean"):
        assert r4[k][:, :8].tobytes() == r2[k][:, :8].tobytes(), k  # the left tile stopped after batch 2
        assert r4[k][:, 8:].tobytes() != r2[k][:, 8:].tobytes(), k
    assert r4["tile_error"].reshape(-1)[0] == r2["tile_error"].reshape(-1)[0] == 0.0
    assert (r4["passes"][:, :8] == 4).all() and (r4["passes"][:, 8:] == 8).all() and r4["pixel_passes"] == 64 * 4 + 64 * 8
    assert (r4["mean"][:, :8] == F32(1.5)).all() and (r4["mean"][:, 8:] == F32(11.0) / F32(4.0)).all()


def test_checker_per_pixel_counts_on_a_frame_with_edge_tiles():
    import adaptive_checker as A
    w, h = 13, 11  # 2 x 2 tiles, all but the first are edge tiles
    noisy = np.zeros((h, w), F32)
    noisy[8:, 8:] = 1.0  # only the corner tile (5 x 3 pixels) stays noisy
    batches = [(np.ones((h, w), F32), noisy)] * 3
    r = A.adaptive(_hand(batches, w, h), w, h, 2, 2, 1, 6, threshold=0.1)
    assert r["batches"] == 3 and [a.tolist() for a in r["active"]] == [[3]] * 3
    want = np.full((h, w), 2, np.uint32)
    want[8:, 8:] = 6
    assert np.array_equal(r["passes"], want) and r["pixel_passes"] == 2 * (w * h - 15) + 6 * 15
    assert A.tile_mask([3], w, h).sum() == 15


def test_checker_an_error_equal_to_the_threshold_is_not_active_and_select_on_special_values():
    import adaptive_checker as A
    import noise_checker as N
    w, h = 16, 8
    noisy = np.zeros((h, w), F32)
    noisy[:, 8:] = 1.0
    batches = [(np.ones((h, w), F32), 0.5 * noisy)] * 3
    first = A.adaptive(_hand(batches, w, h), w, h, 2, 2, 1, 2, threshold=np.inf)
    e = float(first["tile_error"].reshape(-1)[1])
    assert e > 0
    at = A.adaptive(_hand(batches, w, h), w, h, 2, 2, 1, 6, threshold=e)
    assert at["batches"] == 1 and at["converged"] and at["active"][0].tolist() == []
    below = A.adaptive(_hand(batches, w, h), w, h, 2, 2, 1, 6, threshold=float(np.nextafter(F32(e), F32(0))))
    assert below["active"][0].tolist() == [1]
    plane = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.5, 0.25], F32)
    assert A.select(plane, 0.0).tolist() == [1, 5, 6]
    assert A.select(plane, -1.0).tolist() == [1, 3, 4, 5, 6]
    assert A.select(plane, 0.25).tolist() == [1, 5]
    assert A.select(plane, np.inf).tolist() == [] and A.select(plane, -np.inf).tolist() == [1, 3, 4, 5, 6]
    assert A.select(plane, 0.5).dtype == np.uint32
