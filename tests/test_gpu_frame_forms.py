"""The two-sphere kernels' scatter frame and ray normalisation (csrc/rt_shade.h coord_from_z_pair; csrc/rt_intersect.h ray_new's
normalisation through the one-pair quotient; the switches lean_frame_form and lean_ray_norm_short of csrc/rt_lean.h).
(a) rt_selftest_frame_forms: each site next to the plain operators ON the device -- over the host check's own edge grid, which must
reach both sides of each guard, and over 2^20 seeded random inputs per site; this is the only test of the frame's cold copy, because
no scene the host accepts sends a sphere normal there.  (b) frames and ray counts of rtweekend1, bit for bit against the general
spheres-only kernel and against the oracle as tests/test_gpu_parity.py compares frames.  tests/test_frame_forms_host.py runs the
frame's algebra on the CPU."""
import numpy as np
import pytest

import host_check
import scenes
from gpu_support import abi, assert_same_bits
from test_gpu_parity import assert_images_match  # the parity tests' own comparison and tolerance

pytestmark = pytest.mark.gpu

N_RANDOM = 1 << 20


@pytest.fixture(scope="module")
def edge_grid(tmp_path_factory):
    """(n, 3) f32: the edge grid of tests/cpp/frame_forms_check.cpp, written out by that program itself (host code only, built
    here without the sanitizers), so that host and device run the very same operands"""
    return host_check.edge_grid("frame_forms_check", 3, tmp_path_factory)


def _jittered_unit_normals(n):
    """seeded unit normals, each component moved by up to +-4 ulps: what a hit record holds after its own roundings"""
    rng = np.random.default_rng(20261021)
    v = rng.normal(size=(n, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    bits = v.view(np.int32) + rng.integers(-4, 5, (n, 3), dtype=np.int32)  # (no component of these is within 4 ulps of zero)
    return bits.view(np.float32)


def _directions(n):
    """seeded directions with component magnitudes log-uniform over [2^-62, 2^22], either sign: both sides of ray_new's bounds"""
    rng = np.random.default_rng(20261022)
    mag = 2.0 ** rng.uniform(-62.0, 22.0, (n, 3))
    return (mag * rng.choice((-1.0, 1.0), (n, 3))).astype(np.float32)


def test_both_sites_return_the_plain_operators_bits_on_the_device(hb, edge_grid):
    res = hb.selftest_frame_forms(edge_grid)
    print("edge grid:", res)
    assert res["tested"] == len(edge_grid) == 32 ** 3, res
    assert res["frame_mismatches"] == 0 and res["ray_mismatches"] == 0, res
    # the grid reaches both sides of each guard: the short forms and the plain copies both ran
    assert res["frame_short"] > 0 and res["frame_plain"] > 0 and res["ray_short"] > 0 and res["ray_plain"] > 0, res
    # what the kernels' switches select: every form named here is a form the counts above are about
    assert set(res["in_use"]) <= set(abi.FRAME_FORM_NAMES), res
    normals = _jittered_unit_normals(N_RANDOM)
    assert np.abs(normals).min() > 0.0
    res = hb.selftest_frame_forms(normals)
    print("jittered unit normals:", res)
    assert res["tested"] == N_RANDOM and res["frame_mismatches"] == 0 and res["ray_mismatches"] == 0, res
    assert res["frame_plain"] < N_RANDOM // 1000, res  # the cold copy stays cold on what a render feeds it
    res = hb.selftest_frame_forms(_directions(N_RANDOM))
    print("directions:", res)
    assert res["tested"] == N_RANDOM and res["frame_mismatches"] == 0 and res["ray_mismatches"] == 0, res
    assert res["ray_short"] > 0 and res["ray_plain"] > 0, res
    with pytest.raises(hb.RtHipError):
        hb.selftest_frame_forms(edge_grid, device=99)


@pytest.fixture(scope="module")
def loaded(hb, O):
    ls = scenes.load_ssml("rtweekend1")
    general = hb.HipScene(ls.scene, device=0)
    general.set_tuning(abi.RT_TUNE_FEATURE_SET, 0)
    return hb.HipScene(ls.scene, device=0), general, O.Scene(ls.scene), ls.camera_params


@pytest.mark.parametrize("split", [1, 4])
def test_rtweekend1_frames_keep_their_bits(hb, O, loaded, split):
    pair, general, cpu, params = loaded
    opts = abi.default_render_opts(96, 54, 16, method=abi.RT_METHOD_MIS, seed=29)
    opts.max_depth = 50
    opts.sample_split = split
    cam = hb.camera_new(**params)
    img, rays = pair.render(cam, opts)
    assert "rt::FeatPair" in pair.last_launch_info()["kernel"], pair.last_launch_info()
    img_g, rays_g = general.render(cam, opts)
    assert "rt::Feat<false, false, false, false>" in general.last_launch_info()["kernel"], general.last_launch_info()
    ref, ref_rays = cpu.render(O.camera_new(**params), opts)
    assert_same_bits(img, img_g, f"split={split}: against the general spheres-only kernel", nan_equal=False)
    assert rays == rays_g, (split, rays, rays_g)
    assert_images_match(img, ref, f"split={split}: against the oracle")
    assert rays == ref_rays, (split, rays, ref_rays)
