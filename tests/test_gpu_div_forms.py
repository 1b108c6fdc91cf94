"""The one-pair f32 quotient of csrc/rt_lean.h (lean_div_core_gfx950) rests on gfx950's refined reciprocal being RN(1 / d): a fact
about one chip, settled by enumeration ON it.  rt_selftest_div_forms runs the one-pair form, the two-pair form and `n / d` side by
side; the whole 2^23 x 2^23 run is profiles/r09_div_forms_enumeration.txt, and this file asserts on every build the slice that is
most likely to differ (denominators at the ends of the significand range, around 1.5 and sqrt 2, 54 seeded ones; the exponent
pairs at the ends of the tame range and at the bounds the call sites test), the wrappers on special numerators, the guarded call
sites on operands on both sides of every bound, sky_pdf as the two-sphere kernels instantiate it against the default instantiation
on every table regime, and frames against the general kernel and the oracle."""
import numpy as np
import pytest

import div_forms_cases
import scenes
import sky_cases
from gpu_support import abi, assert_same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32

DENOMINATORS, EXPONENTS = div_forms_cases.DENOMINATORS, list(div_forms_cases.EXPONENTS)


def test_the_form_in_use_is_the_quotient_on_the_slice(hb):
    assert DENOMINATORS.size == 64
    res = hb.selftest_div_forms(DENOMINATORS, EXPONENTS)
    print(res)
    assert res["tested"] == len(EXPONENTS) * DENOMINATORS.size << 23
    assert set(res["forms"]) == set(abi.DIV_FORM_NAMES) and len(res["in_use"]) == 1
    for name in res["in_use"]:
        bad, first = res["forms"][name]
        assert bad == 0 and first is None, (name, bad, None if first is None else tuple(hex(x) for x in first))
    assert res["forms"]["two_pairs"] == (0, None)  # hipcc's own expansion minus its identity steps
    # a range is the list of its members
    by_range = hb.selftest_div_forms(None, [(0, 0), (3, -2)], first_denominator=0x7FFFF0, n_denominators=16)
    by_list = hb.selftest_div_forms(np.arange(0x7FFFF0, 0x800000, dtype=np.uint32), [(0, 0), (3, -2)])
    assert by_range == by_list and by_range["tested"] == 2 * 16 << 23


def _pairs(values):
    v = np.asarray(values, dtype=F32)
    return np.stack(np.meshgrid(v, v, indexing="ij"), -1).reshape(-1, 2)


def _around(x):
    x = F32(x)
    return [np.nextafter(x, F32(0)), x, np.nextafter(x, F32(np.inf))]


def test_the_fix_wrappers_on_special_numerators(hb):
    lo, hi = 2.0 ** -81, 2.0 ** 41
    numerators = [0.0, -0.0, np.inf, -np.inf, np.nan, lo, -lo, hi, -hi]
    denominators = [lo, -lo, hi, -hi, 2.0 ** -54, 2.0 ** 14, 1.0, np.nextafter(F32(2.0), F32(0)), np.nextafter(F32(hi), F32(0))]
    ops = np.array([(n, d) for n in numerators for d in denominators], dtype=F32)
    res = hb.selftest_div_forms(operands=ops)
    print(res)
    # every special numerator is in the domain with every denominator, and each tame end with the denominators less than 96 exponents away
    assert res["tested"] == len(ops) and res["in_domain"] >= 5 * len(denominators) + 4 * 3
    assert res["sites"]["fix"] == 0 and res["sites"]["div3_fix"] == 0, res


def test_guarded_sites_take_the_plain_operator_outside_their_bounds(hb):
    """no scene the host accepts reaches most of these lanes, so the self-test feeds the site functions directly: operands just
    inside and just outside every bound the sites and the forms have, zeros, denormals, infinities and NaN, in every pairing"""
    edges = []
    for e in (-81, -75, -54, -27, 14, 20, 41):
        edges += _around(2.0 ** e) + [-F32(2.0 ** e)]
    edges += _around(2.0 ** -95) + _around(2.0 ** 96 * 2.0 ** -81)  # exponents 95 / 96 away from 2^-81 ...
    edges += [2.0 ** -14, 2.0 ** -13, 2.0 ** 81, 2.0 ** 82]        # ... and pairs 95 / 96 apart among themselves
    edges += [0.0, -0.0, 1e-45, -1e-45, 1e-40, 2.0 ** -126, np.nextafter(F32(2.0 ** -126), F32(0)), 3e38, np.inf, -np.inf, np.nan, 1.0, -3.0, 0.1, 0.5]
    ops = _pairs(edges)
    res = hb.selftest_div_forms(operands=ops)
    print(res)
    assert res["tested"] == len(ops) and 0 < res["in_domain"] < len(ops)
    assert res["sites"] == {name: 0 for name in abi.DIV_SITE_NAMES}, res
    # ... and seeded random bit patterns of every class, and random operands of a render's magnitudes
    rng = np.random.default_rng(11)
    rnd = rng.integers(0, 1 << 32, size=(1 << 16, 2), dtype=np.uint64).astype(np.uint32).view(F32)
    res = hb.selftest_div_forms(operands=rnd)
    assert res["tested"] == len(rnd) and res["sites"] == {name: 0 for name in abi.DIV_SITE_NAMES}, res
    usual = np.exp2(rng.uniform(-30, 12, size=(1 << 16, 2))).astype(F32)
    res = hb.selftest_div_forms(operands=usual)
    assert res["in_domain"] == len(usual) and res["sites"] == {name: 0 for name in abi.DIV_SITE_NAMES}, res


def test_arguments_are_checked(hb):
    with pytest.raises(hb.RtHipError):
        hb.selftest_div_forms(DENOMINATORS, [(0, 0)], device=99)
    with pytest.raises(hb.RtHipError):
        hb.selftest_div_forms(DENOMINATORS, [(0, 128)])
    with pytest.raises(hb.RtHipError):
        hb.selftest_div_forms(None, [(0, 0)], first_denominator=0x7FFFFF, n_denominators=2)
    with pytest.raises(hb.RtHipError):
        hb.selftest_div_forms(None, [(0, 0)] * 3, first_denominator=0, n_denominators=1 << 16)
    with pytest.raises(hb.RtHipError):
        hb.selftest_div_forms(operands=np.zeros((0, 2), dtype=F32))


@pytest.mark.parametrize("name", sorted(sky_cases.CASES))
def test_sky_pdf_of_the_pair_kernels_is_the_default_instantiation(hb, name):
    gpu = hb.HipScene(sky_cases.sky_only(name), device=0)
    rng = np.random.default_rng(13)
    v = rng.normal(size=(4096, 3))
    unit = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    zeroed = unit[:96].copy()  # a zero component each
    zeroed[np.arange(96), np.arange(96) % 3] = 0.0
    dirs = np.concatenate([sky_cases.chosen_directions(name), unit, zeroed])  # (poles, cell borders, the seam: chosen_directions)
    pair, default = hb.selftest_sky_pdf_forms(gpu, dirs)
    assert pair.tobytes() == default.tobytes()
    # ... and the default instantiation is the one rt_selftest_sky runs
    _, _, listed = gpu.selftest_sky(0, 0, dirs=dirs)
    assert_same_bits(default, listed, name, nan_equal=False)
    assert np.isfinite(default).any()


def two_spheres_under(case):
    sc = scenes.SceneDescription()
    sc.sphere((0.0, -100.5, -1.0), 100.0, sc.lambertian(sc.solid((0.5, 0.5, 0.5)), 0.5))
    sc.sphere((0.0, 0.0, -1.0), 0.5, sc.lambertian(sc.solid((0.7, 0.3, 0.3)), 0.5))
    return sky_cases.with_sky(sc, case)


FRAME_CAMERA = dict(origin=(0.0, 0.0, 1.0), lookat=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0), fov=50.0, aspect_ratio=float(F32(16.0) / F32(9.0)),
                    aperture=0.0, focus_dist=10.0)


def _frame_scenes():
    ls = scenes.load_ssml("rtweekend1")
    return {"rtweekend1": (ls.scene, ls.camera_params), "zero_pdf_cells": (two_spheres_under("black"), FRAME_CAMERA)}


@pytest.mark.parametrize("which", ["rtweekend1", "zero_pdf_cells"])
def test_frames_of_the_pair_kernel_keep_the_general_kernels_and_the_oracles_bytes(hb, O, which):
    sc, cam = _frame_scenes()[which]
    pair, general, cpu = hb.HipScene(sc, device=0), hb.HipScene(sc, device=0), O.Scene(sc)
    general.set_tuning(abi.RT_TUNE_FEATURE_SET, 0)
    opts = abi.default_render_opts(64, 36, 16, method=abi.RT_METHOD_MIS, seed=7)
    img, rays = pair.render(hb.camera_new(**cam), opts)
    assert "rt::FeatPair" in pair.last_launch_info()["kernel"], pair.last_launch_info()["kernel"]
    img_g, rays_g = general.render(hb.camera_new(**cam), opts)
    assert "rt::FeatPair" not in general.last_launch_info()["kernel"]
    ref, ref_rays = cpu.render(O.camera_new(**cam), opts)
    assert_same_bits(img, img_g, which + " against the general kernel", nan_equal=False)
    assert_same_bits(img, ref, which + " against the oracle", nan_equal=False)
    assert rays == rays_g == ref_rays
