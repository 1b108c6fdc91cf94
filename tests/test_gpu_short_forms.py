"""The short forms of csrc/rt_lean.h that rest on what gfx950's v_rcp_f32 / v_sqrt_f32 return (not on what any 1-ulp approximation
would): rt_selftest_short_forms enumerates them against the plain operators ON the device -- every significand of both signs at
eight exponents across the tame range for 1 / d, every float of lean_sqrt's domain for sqrtf -- and every form the render kernels
use must show no mismatch.  The call sites that guard them (Ray::new of the two-sphere and of the general kernels) must send
operands outside the forms' domains through the plain operators; frames of the kernels that use the forms keep the oracle's bits;
axis-parallel and tiny-component rays keep the oracle's hit records."""
import numpy as np
import pytest

import scenes
from gpu_support import abi, assert_same_bits

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 40, 16
RCP_INPUTS = 8 * 2 * (1 << 23)                    # eight exponents, both signs, every significand
SQRT_INPUTS = (1 << 32) - (0x0F800000 - 1) - ((1 << 23) - 1)  # every bit pattern but the positives below 2^-96 and the negative denormals


@pytest.fixture(scope="module")
def enumeration(hb):
    return hb.selftest_short_forms(0)


def test_every_form_in_use_is_exact_over_the_whole_enumeration(enumeration):
    forms, raw = enumeration["forms"], enumeration["sqrt_raw"]
    print(enumeration)
    assert set(forms) == set(abi.SHORT_FORM_NAMES)
    for name, (tested, bad, first) in forms.items():
        assert tested == (SQRT_INPUTS if name.startswith("sqrt") else RCP_INPUTS), (name, tested)
    assert sum(raw.values()) == SQRT_INPUTS and raw["other"] == 0, raw  # v_sqrt_f32 is within one ulp, as documented
    # the two forms that are hipcc's own expansions minus identity steps, and whatever else the kernels use
    assert {"rcp_refined", "inv_two_pairs", "sqrt_both"} <= set(enumeration["in_use"])
    for name in enumeration["in_use"]:
        tested, bad, first = forms[name]
        assert bad == 0 and first is None, (name, bad, None if first is None else hex(first))


def test_first_mismatch_is_reported_for_a_form_that_has_one(enumeration):
    """the raw instructions are NOT the operators (that is why the forms exist): the report names a real input for them"""
    tested, bad, first = enumeration["forms"]["sqrt_raw"]
    raw = enumeration["sqrt_raw"]
    assert bad == raw["high"] + raw["low"] and raw["high"] > 0 and raw["low"] > 0  # both corrections of lean_sqrt are needed on this chip
    x = np.array([first], dtype=np.uint32).view(np.float32)[0]
    assert x >= np.float32(2.0 ** -96) and np.isfinite(x), hex(first)


def test_call_sites_send_out_of_domain_operands_through_the_plain_operators(hb):
    ops = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-39, 2.0 ** -126, 2.0 ** -100, -2.0 ** -100, 2.0 ** -61, np.nextafter(np.float32(2.0 ** -60), np.float32(0)),
           2.0 ** -60, 2.0 ** -59, 2.0 ** 20, 2.0 ** 21, 2.0 ** 60, -2.0 ** 60, 3e38, np.inf, -np.inf, np.nan, 1.0, -3.0, 0.1]
    res = hb.selftest_short_forms(0, np.array(ops, dtype=np.float32))
    assert res["tested"] == 4 * len(ops)
    assert res["sites"] == {name: 0 for name in abi.SHORT_SITE_NAMES}, res
    # ... and on seeded random bit patterns of every class
    rnd = np.random.default_rng(7).integers(0, 1 << 32, size=1 << 16, dtype=np.uint64).astype(np.uint32).view(np.float32)
    res = hb.selftest_short_forms(0, rnd)
    assert res["tested"] == 4 * rnd.size and res["sites"] == {name: 0 for name in abi.SHORT_SITE_NAMES}, res


def test_arguments_are_checked(hb):
    with pytest.raises(hb.RtHipError):
        hb.selftest_short_forms(99)
    with pytest.raises(hb.RtHipError):
        hb.selftest_short_forms(0, np.zeros(0, dtype=np.float32))


@pytest.fixture(scope="module")
def loaded(hb, O):
    ls = scenes.load_ssml("rtweekend1")
    general = hb.HipScene(ls.scene, device=0)
    general.set_tuning(abi.RT_TUNE_FEATURE_SET, 0)
    return ls, hb.HipScene(ls.scene, device=0), general, O.Scene(ls.scene)


CASES = {  # name -> (method, sample_split, max_depth)
    "mis": (abi.RT_METHOD_MIS, 1, 50),
    "mis split 4": (abi.RT_METHOD_MIS, 4, 50),
    "naive": (abi.RT_METHOD_NAIVE, 1, 50),
    "mis depth 8": (abi.RT_METHOD_MIS, 1, 8),
}


@pytest.fixture(scope="module")
def references(O, loaded):
    """the oracle's frame and ray count of every case, computed once"""
    ls, _, _, cpu = loaded
    out = {}
    for name, (method, split, depth) in CASES.items():
        opts = _opts(method, split, depth)
        out[name] = cpu.render(O.camera_new(**ls.camera_params), opts)
    return out


def _opts(method, split, depth):
    opts = abi.default_render_opts(W, H, SPP, method=method, seed=5)
    opts.sample_split = split
    opts.max_depth = depth
    return opts


@pytest.mark.parametrize("forced_general", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_frames_keep_the_oracles_bytes(hb, loaded, references, case, forced_general):
    ls, pair, general, _ = loaded
    gpu = general if forced_general else pair
    img, rays = gpu.render(hb.camera_new(**ls.camera_params), _opts(*CASES[case]))
    kernel = gpu.last_launch_info()["kernel"]
    assert ("rt::Feat<false, false, false, false>" if forced_general else "rt::FeatPair") in kernel, kernel
    ref, ref_rays = references[case]
    assert_same_bits(img, ref, f"{case} ({kernel})", nan_equal=False)
    assert rays == ref_rays, (case, rays, ref_rays)


def test_axis_parallel_and_tiny_component_rays_keep_the_oracles_hit_records(hb, loaded):
    """Ray::new's guard: a zero component (1 / 0 = inf must come from the plain operator) and a component below 2^-60"""
    _, pair, _, cpu = loaded
    tiny = float(np.float32(2.0 ** -70))
    origins = [(0.0, 0.0, 0.0)] * 8
    directions = [(0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (-0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (tiny, 1.0, 0.0), (tiny, 1.0, -tiny), (0.25, 1.0, tiny),
                  (tiny, 1.0, -0.125)]
    got, ref = pair.check_hit(origins, directions), cpu.check_hit(origins, directions)
    assert got.tobytes() == ref.tobytes()
    assert got["found"].any()
