"""The kernels' sky sampling and pdf on every table regime of tests/sky_cases.py (test_sky_tables.py shows on the CPU that each case
is in its regime): rt_selftest_sky -- sky_sample and sky_pdf as the render kernels inline them -- against the oracle over 65 536
streams and the chosen directions, with the tables in global memory and staged in LDS; the tie cases over 2^21 streams; 32 x 18
renders of three scenes (one per feature set) under every traversal mode, the fine schedule and a captured graph; and where the
launch planner puts the tables.  Every comparison is on bits."""
import functools

import numpy as np
import pytest

import scenes
import sky_cases as SK
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture

pytestmark = pytest.mark.gpu
abi = scenes.abi
NAMES = list(SK.CASES)
RENDER_PAIRS = [(scene, name) for scene in SK.RENDER_SCENES for name in SK.RENDER_CASES]


def _placements(name):
    return (0, 1) if SK.CASES[name].fits_lds else (0,)


@functools.lru_cache(maxsize=None)
def _oracle_selftest(O, name, n, seed):
    """(directions of streams 0..n-1, pdf at each, pdf at the chosen directions) by the oracle, once per case"""
    cpu = O.Scene(SK.sky_only(name))
    dirs = cpu.sample_directions(2, n, seed=seed)
    out = dirs, cpu.eval_pdfs(2, dirs), cpu.eval_pdfs(2, SK.chosen_directions(name))
    for a in out:
        a.setflags(write=False)
    return out


def _check_selftest(hb, O, name, n, seed):
    gpu = hb.HipScene(SK.sky_only(name), device=0)
    info = gpu.sky_info()
    assert info["guide_k"] == SK.CASES[name].guide_k and (info["table_bytes"] <= SK.LDS_LIMIT) == SK.CASES[name].fits_lds
    ref_dirs, ref_pdf_s, ref_pdf = _oracle_selftest(O, name, n, seed)
    for lds in _placements(name):
        dirs, pdf_s, pdf = gpu.selftest_sky(lds, n, seed=seed, dirs=SK.chosen_directions(name))
        what = f"{name} tables {'in LDS' if lds else 'in global memory'}"
        assert_same_bits(dirs, ref_dirs, f"{what}: sampled directions", nan_equal=True)
        assert_same_bits(pdf_s, ref_pdf_s, f"{what}: pdf at the sampled directions", nan_equal=True)
        assert_same_bits(pdf, ref_pdf, f"{what}: pdf at the chosen directions", nan_equal=True)
    if not SK.CASES[name].fits_lds:
        with pytest.raises(hb.RtHipError) as e:
            gpu.selftest_sky(1, 16, seed=seed)
        assert e.value.code == abi.RT_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", NAMES)
def test_selftest_matches_the_oracle(hb, O, name):
    _check_selftest(hb, O, name, SK.SELFTEST_N, SK.SELFTEST_SEED)


@pytest.mark.parametrize("name", SK.TIE_CASES)
def test_ties(hb, O, name):
    """TIE_N streams: test_sky_tables.py counts the draws among them that equal a CDF entry (23 and 17 searches)"""
    _check_selftest(hb, O, name, SK.TIE_N, SK.TIE_SEED)


def test_selftest_refuses_what_it_cannot_run(hb):
    sc = SK.unsampled(SK.sky_only("control"), "control")
    with pytest.raises(hb.RtHipError) as e:
        hb.HipScene(sc, device=0).selftest_sky(0, 16)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(hb.RtHipError) as e:
        hb.HipScene(SK.sky_only("control"), device=abi.RT_DEVICE_NONE).selftest_sky(0, 16)
    assert e.value.code == abi.RT_ERR_NO_DEVICE


# ---- renders ----
def _opts(method=abi.RT_METHOD_MIS):
    return abi.default_render_opts(SK.W, SK.H, SK.SPP, method=method, seed=SK.SEED)


def _scene(scene, name):
    sc, cam_params = SK.RENDER_SCENES[scene]()
    return SK.with_sky(sc, name), cam_params


@functools.lru_cache(maxsize=None)
def _oracle_frame(O, scene, name):
    sc, cam_params = _scene(scene, name)
    img, rays = O.Scene(sc).render(O.camera_new(**cam_params), _opts())
    img.setflags(write=False)
    return img, rays


@pytest.mark.parametrize("scene,name", RENDER_PAIRS, ids=[f"{scene}.{name}" for scene, name in RENDER_PAIRS])
def test_render_matches_the_oracle(hb, O, scene, name):
    sc, cam_params = _scene(scene, name)
    gpu, cam = hb.HipScene(sc, device=0), hb.camera_new(**cam_params)
    ref, ref_rays = _oracle_frame(O, scene, name)
    try:
        for mode in (0, 1, -1):
            gpu.set_traversal(mode)
            img, rays = gpu.render(cam, _opts())
            assert_same_bits(img, ref, f"{scene} under {name}, traversal {mode}", nan_equal=True)
            assert rays == ref_rays
            info = gpu.last_launch_info()
            if not SK.CASES[name].fits_lds:
                assert info["sky_in_lds"] == 0, (scene, name, mode)
    finally:
        gpu.set_traversal(-1)
    # NAIVE never reads the tables: the frame of the same sky without a sampler
    naive, naive_rays = gpu.render(cam, _opts(abi.RT_METHOD_NAIVE))
    assert gpu.last_launch_info()["sky_in_lds"] == 0
    plain_sc, _ = SK.RENDER_SCENES[scene]()
    plain = hb.HipScene(SK.unsampled(plain_sc, name), device=0)
    ref_naive, ref_naive_rays = plain.render(cam, _opts(abi.RT_METHOD_NAIVE))
    assert_same_bits(naive, ref_naive, f"{scene} under {name}, NAIVE against sampler_res (0, 0)", nan_equal=True)
    assert naive_rays == ref_naive_rays


def test_sky_in_lds_takes_both_values(hb):
    """one automatic MIS launch of the 30 spheres under every case: which tables the planner staged"""
    staged = {}
    for name in SK.RENDER_CASES:
        sc, cam_params = _scene("spheres", name)
        gpu = hb.HipScene(sc, device=0)
        gpu.render(hb.camera_new(**cam_params), _opts())
        staged[name] = gpu.last_launch_info()["sky_in_lds"]
    print("sky tables in LDS:", sorted(n for n, v in staged.items() if v))
    print("sky tables in global memory:", sorted(n for n, v in staged.items() if not v))
    assert set(staged.values()) == {0, 1}
    assert all(staged[n] == 0 for n in SK.BIG + SK.HUGE) and staged["control"] == 1


def test_deep_tree_keeps_the_sky_where_the_planner_says(hb, O):
    """the 112-sphere chain under a 100 x 100 sky: the launch reports where its tables are, and the frame is the oracle's"""
    sc = scenes.skewed_chain_of_spheres(112, ratio=1.44)
    sc.set_sky(sc.lerp(*SK.LERP), (100, 100))
    gpu, cam = hb.HipScene(sc, device=0), hb.camera_new(**scenes.CHAIN_CAMERA)
    ref, ref_rays = O.Scene(sc).render(O.camera_new(**scenes.CHAIN_CAMERA), _opts())
    img, rays = gpu.render(cam, _opts())
    info = gpu.last_launch_info()
    assert_same_bits(img, ref, "chain under a 100 x 100 sky", nan_equal=True)
    assert rays == ref_rays
    tables = SK.table_bytes(100, 100, 128)
    assert gpu.sky_info()["table_bytes"] == tables <= SK.LDS_LIMIT
    print(f"chain: sky_in_lds={info['sky_in_lds']} lds_bytes={info['lds_bytes']} fine={info['fine']} kernel={info['kernel']}")
    # The planner stages the tables unless that costs a resident workgroup (csrc/rt_api.cpp).  This coarse launch keeps the whole
    # worst-case stack of the wide tree in LDS: 85 entries x 4 waves x 256 B = 87 040 B, so one workgroup fits the 160 KB of a CU
    # with or without the tables, and they are staged: 53 732 B padded to 53 744 behind the stacks.  (Measured on an MI355X:
    # sky_in_lds = 1, lds_bytes = 140 784.)  A planner that changes its occupancy rule, or a tree whose stacks grow, fails here.
    depth = gpu.wide_tree()[2]
    staged = 4 * ((100 * 101 + 101 + 3) // 4 * 4) + 101 * 128
    assert info["fine"] == 0 and info["pruned"] == 1 and info["blocks_per_cu"] == 1
    assert info["sky_in_lds"] == 1
    assert info["lds_bytes"] == info["block_threads"] // 64 * depth * 256 + staged == 87040 + 53744


@pytest.mark.parametrize("name", ("control", "unguided_wide", "big_guided", "plateaus"))
def test_fine_schedule(hb, O, name):
    sc, cam_params = _scene("spheres", name)
    gpu, cam = hb.HipScene(sc, device=0), hb.camera_new(**cam_params)
    ref, ref_rays = _oracle_frame(O, "spheres", name)
    gpu.set_tuning(abi.RT_TUNE_SCHEDULE, 1)
    try:
        img, rays = gpu.render(cam, _opts())
        info = gpu.last_launch_info()
    finally:
        gpu.set_tuning(abi.RT_TUNE_SCHEDULE, -1)
    assert info["fine"] == 1 and info["pruned"] == 1
    assert_same_bits(img, ref, f"spheres under {name}, fine schedule", nan_equal=True)
    assert rays == ref_rays


def test_graph_captured_render(hb, O):
    import torch
    sc, cam_params = _scene("spheres", "unguided_wide")
    gpu, cam = hb.HipScene(sc, device=0), hb.camera_new(**cam_params)
    ref, _ = _oracle_frame(O, "spheres", "unguided_wide")
    run = GuardedBuffers(torch, {"frame": ((SK.H, SK.W, 3), np.float32)})
    g = capture(torch, lambda stream: gpu.render_device(cam, _opts(), run.ptr("frame"), stream=stream))
    assert run.untouched("frame")  # capture ran nothing
    for _ in range(2):
        run.refill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(run.read("frame"), ref, "unguided_wide, graph replay", nan_equal=True)


def test_no_side_effects_on_render(hb):
    sc, cam_params = _scene("spheres", "control")
    gpu, cam = hb.HipScene(sc, device=0), hb.camera_new(**cam_params)
    assert_render_unaffected(gpu, cam, lambda opts, img: [gpu.selftest_sky(lds, 4096, dirs=SK.chosen_directions("control")) for lds in (0, 1)])
