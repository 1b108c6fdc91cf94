"""Without a GPU: (1) every off-default option value of tests/post_options_cases.py changes the checker's result on the synthetic
input it is paired with -- by at least 100 x TOL in denoise_checker.relative_error for the stages held to a tolerance, by at least
one byte or a state field for the bit-exact ones -- so that tests/test_gpu_post_options.py, which runs exactly these pairs on the
kernels, cannot pass with an option ignored; (2) the table itself covers every option on both sides of its default; (3) the history
planes of rt_denoise_temporal are indexed in 64 bits (a frame of more than 2^32 / 3 pixels cannot be run in a test)."""
import os
import re

import pytest

import post_options_cases as P
import scenes

abi = scenes.abi


@pytest.mark.parametrize("case", P.DENOISE_CASES, ids=[c[0] for c in P.DENOISE_CASES])
def test_denoise_option_moves_the_checker(case):
    _, opts = case
    s = P.denoise_sensitivity(P.denoise_synthetic(), opts)
    print(f"denoise {case[0]}: {s:.3e}")
    assert s >= P.SENSITIVITY, s


@pytest.mark.parametrize("case", P.TEMPORAL_CASES, ids=[c[0] for c in P.TEMPORAL_CASES])
def test_temporal_option_moves_the_checker(hb, case):
    name, kind, frames, opts = case
    s = P.temporal_sensitivity(hb, kind, frames, opts)
    print(f"temporal {name}: " + " ".join(f"{k} {v:.3e}" for k, v in s.items()))
    assert max(s.values()) >= P.SENSITIVITY, s
    # what each option is for must move, not only something
    for k in opts:
        if k in P.SIGMAS or k in ("alpha_color", "depth_tolerance", "normal_tolerance"):
            assert s["out"] >= P.SENSITIVITY, (k, s)
        elif k == "alpha_moments":
            assert max(s["m1"], s["m2"]) >= P.SENSITIVITY, (k, s)
        elif k == "max_history":
            assert s["n"] >= P.SENSITIVITY, (k, s)


def test_temporal_tolerances_flip_taps_both_ways(hb):
    """depth_tolerance and normal_tolerance: some pixels keep their history and some lose it at every value of the table"""
    for name, kind, frames, opts in P.TEMPORAL_CASES:
        if not {"depth_tolerance", "normal_tolerance"} & set(opts) or name == "all":
            continue
        n = P.temporal_checker_sequence(hb, kind, frames, opts)["n"]
        n0 = P.temporal_checker_sequence(hb, kind, frames, {})["n"]
        kept, lost = float((n > 1).mean()), float((n == 1).mean())
        print(f"{name}: history kept at {kept:.3f} of the pixels, restarted at {lost:.3f}; differs from the default at "
              f"{float((n != n0).mean()):.3f}")
        assert kept > 0.02 and lost > 0.02 and (n != n0).mean() > 0.02, name


@pytest.mark.parametrize("case", P.DISPLAY_CASES, ids=[c[0] for c in P.DISPLAY_CASES])
def test_display_option_moves_the_checker(O, case):
    name, key, opts = case
    img = P.display_image(key)
    for label, state in P.DISPLAY_STATES:
        bytes_differ, ev_differs = P.display_differs(O, img, state, opts)
        assert bytes_differ and ev_differs, (name, label)


def test_display_clamps_really_clamp(O):
    import display_checker as D
    for name, key, opts in P.DISPLAY_CASES:
        if not name.startswith("ev_"):
            continue
        hist, _ = D.histogram(P.display_image(key))
        free = float(D.DEFAULTS["key_ev"]) - float(D.meter(hist, 0.10, 0.90))
        ev = float(D.exposure(hist, None, **opts)[0])
        print(f"{name}: unclamped target {free:.3f}, exposure {ev:.3f}")
        if name == "ev_min_lower":  # the default clamps, the value frees the target
            assert free < -16.0 and ev == pytest.approx(free, abs=1e-5)
        else:
            bound = opts.get("ev_min", opts.get("ev_max"))
            assert ev == bound and ((free < bound) if "ev_min" in opts else (free > bound))


@pytest.mark.parametrize("case", P.UPSCALE_CASES, ids=[c[0] for c in P.UPSCALE_CASES])
def test_upscale_option_moves_the_checker(O, case):
    _, opts = case
    for make in P.UPSCALE_SYNTHETIC.values():
        color, src, dst, W, H = make()
        assert P.upscale_differs(O, color, src, dst, W, H, opts)


def test_the_table_covers_every_option_on_both_sides(hb):
    import ctypes as C

    def sides(values, default):
        return any(v < default for v in values), any(v > default for v in values)

    def single(cases, option):
        return [c[-1][option] for c in cases if set(c[-1]) == {option}]

    d = abi.DenoiseOpts()
    hb.lib().rt_denoise_opts_default(C.byref(d))
    t = hb.temporal_opts(2, 2)
    for k in P.SIGMAS:
        assert sides(single(P.DENOISE_CASES, k), getattr(d, k)) == (True, True), k
        assert sides(single(P.TEMPORAL_CASES, k), getattr(d, k)) == (True, True), k
    for k in abi.TEMPORAL_OPTIONS:
        assert sides(single(P.TEMPORAL_CASES, k), getattr(t, k)) == (True, True), k
    o = hb.display_opts(1, 1)
    for k in ("key_ev", "meter_low", "meter_high", "ev_min"):
        assert sides(single(P.DISPLAY_CASES, k), getattr(o, k)) == (True, True), k
    assert sides(single(P.DISPLAY_CASES, "ev_max"), o.ev_max) == (True, False)  # see the module text of post_options_cases
    u = hb.upscale_opts(2, 2, 2, 2)
    for k in abi.UPSCALE_OPTIONS:
        assert sides(single(P.UPSCALE_CASES, k), getattr(u, k)) == (True, True), k
    for cases, n_options in ((P.DENOISE_CASES, 3), (P.TEMPORAL_CASES, 8), (P.DISPLAY_CASES, 5), (P.UPSCALE_CASES, 2)):
        assert any(len(c[-1]) >= n_options for c in cases)  # the combined case


def test_history_planes_are_indexed_in_64_bits(hb):
    """H2 of a history starts 2 * n_px float4 into it: in 32-bit arithmetic `2 * n_px + p` wraps above 2^32 / 3 pixels (1.43 G; the
    API takes 2^31) and lands in H0.  Such a history is 68 GB, so this is held at the source: every index into hist_in / hist_out
    that reaches the third plane multiplies in 64 bits."""
    src = open(os.path.join(scenes.ROOT, "raytracing-rust_amd", "csrc", "rt_temporal.hip")).read()
    third = re.findall(r"hist_(?:in|out)\[\s*2(\w*)\s*\*\s*n_px", src)
    assert len(third) >= 3 and all(suffix == "ull" for suffix in third), third
    assert not re.search(r"hist_(?:in|out)\[[^\]]*\b2u\s*\*", src)
    # and the host still sizes the largest frame the API takes without wrapping
    o = hb.temporal_opts(1 << 16, 1 << 15)
    assert hb.temporal_history_bytes(o) == 48 * (1 << 31) and hb.temporal_workspace_bytes(o) == 32 * (1 << 31)
