"""The carried sky cell of the two-sphere kernels (RT_TUNE_SKY_CELL; csrc/rt_shade.h sky_sample_cell / sky_pdf_carried, the guard
proven per scene by csrc/rt_sky_cell.h).  (a) enumeration on the device: over all 2^24 jitters of an axis at a cell, no guarded lane's
round trip lands in another cell, and the carried pdf is the default's bit for bit; (b) hand-made draws on either side of every
bound of the guard, in waves that are all guarded, all unguarded and mixed -- the only test of the cold region; (c) frames and ray
counts do not depend on the switch and are the oracle's; (d) a sky the host must refuse keeps the flag off."""
import os

import numpy as np
import pytest

import scenes
import sky_cases
from gpu_support import abi, assert_same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
TABLES = ((100, 100), (7, 5))
TWO_SPHERE_CAMERA = dict(origin=(0.0, 0.0, 0.0), lookat=(0.0, 1.0, 0.0), vup=(0.0, 0.0, 1.0), fov=90.0, aspect_ratio=1.0, aperture=0.0, focus_dist=1.0)


def two_spheres(res):
    """a small sphere on a big one under a Lerp sky sampled at `res`: a scene the two-sphere kernels render"""
    sc = scenes.SceneDescription()
    sc.sphere((0.0, 1.0, -100.5), 100.0, sc.lambertian(sc.solid(0.5), 1.0))
    sc.sphere((0.0, 1.0, 0.0), 0.5, sc.lambertian(sc.solid((0.7, 0.3, 0.3)), 0.9))
    sc.set_sky(sc.lerp(*sky_cases.LERP), res)
    return sc


@pytest.fixture(scope="module")
def tables(hb):
    return {res: hb.HipScene(two_spheres(res), device=0) for res in TABLES}


def bits(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def test_the_library_carries_the_cell_where_the_host_proves_the_guard(hb, tables):
    for (rx, ry), g in tables.items():
        _, _, guard = hb.selftest_sky_cell(g, [[0, 0, bits(0.5), bits(0.5)]])
        assert guard["proven"] and guard["enabled"], ((rx, ry), guard)
        assert guard["row_lo"] == 1 and guard["row_hi"] == ry - 2
        assert 0.0 < guard["delta_u"] < 0.25 and 0.0 < guard["delta_v"] < 0.25


@pytest.mark.parametrize("res", TABLES)
def test_no_guarded_jitter_leaves_its_cell(hb, tables, res):
    """the v enumeration on rows 0, row_lo - 1, row_lo, the equator row, row_hi, row_hi + 1 and ry - 1; the u enumeration on columns
    0, rx / 4, rx / 2 and rx - 1 of the equator row and of row_lo.  The raw counts go to profiles/r27_sky_cell_enumeration.txt: this
    table's lines there are replaced by this run's (the counts are a function of the arithmetic alone, so a run that changes the
    file has found a change of the arithmetic)."""
    rx, ry = res
    g = tables[res]
    _, _, guard = hb.selftest_sky_cell(g, [[0, 0, bits(0.5), bits(0.5)]])
    lo, hi = guard["row_lo"], guard["row_hi"]
    runs = [(1, rx // 2, row) for row in sorted({0, lo - 1, lo, ry // 2, hi, hi + 1, ry - 1})]
    runs += [(0, col, row) for row in sorted({ry // 2, lo}) for col in sorted({0, rx // 4, rx // 2, rx - 1})]
    lines = []
    for axis, su, sv in runs:
        _, counts, _ = hb.selftest_sky_cell(g, None, axis=axis, su=su, sv=sv)
        lines.append(f"{rx}x{ry} axis={'uv'[axis]} cell=({su},{sv}) guarded_disagree={counts['guarded_disagree']} unguarded={counts['unguarded']} "
                     f"unguarded_agree={counts['unguarded_agree']} pdf_mismatches={counts['pdf_mismatches']} tested={counts['tested']}")
        print(lines[-1])
        assert counts["tested"] == 1 << 24
        assert counts["guarded_disagree"] == 0 and counts["pdf_mismatches"] == 0, lines[-1]
        guarded_row = lo <= sv <= hi
        if not guarded_row:
            assert counts["unguarded"] == 1 << 24, lines[-1]
        else:  # the margins: with k = delta 2^24 (an integer), the jitters i 2^-24 with i < k or i > 2^24 - k
            delta = guard["delta_u" if axis == 0 else "delta_v"]
            assert counts["unguarded"] == 2 * round(delta * (1 << 24)) - 1, lines[-1]
    _record_enumeration(f"{rx}x{ry} ", lines)


ENUMERATION_FILE = os.path.join(scenes.ROOT, "profiles", "r27_sky_cell_enumeration.txt")


def _record_enumeration(prefix, lines):
    """the file's comment lines, then every table's lines in TABLES' order with this table's replaced"""
    try:
        old = open(ENUMERATION_FILE).read().splitlines() if os.path.exists(ENUMERATION_FILE) else []
        head = [ln for ln in old if ln.startswith("#")]
        body = [ln for ln in old if not ln.startswith("#") and not ln.startswith(prefix)] + lines
        order = [f"{rx}x{ry} " for rx, ry in TABLES]
        body.sort(key=lambda ln: next((k for k, p in enumerate(order) if ln.startswith(p)), len(order)))  # (stable: lines keep their order within a table)
        with open(ENUMERATION_FILE, "w") as f:
            f.write("\n".join(head + body) + "\n")
    except OSError:  # (a read-only checkout: the assertions above are the test)
        pass

def _bound_cases(rx, ry, guard):
    """draws on either side of every bound: the jitters delta and 1 - delta and the next float each way, on each axis, and the rows
    row_lo - 1, row_lo, row_hi, row_hi + 1 -- each of them (the others inside) and each complement (the others outside)"""
    du, dv = F32(guard["delta_u"]), F32(guard["delta_v"])
    one = F32(1.0)

    def around(d):
        lo, hi = F32(d), F32(one - d)
        step = F32(2.0 ** -24)  # the jitters a stream can draw are multiples of it: the bounds' neighbours there, and the next floats
        return [lo - step, np.nextafter(lo, F32(0)), lo, np.nextafter(lo, one), lo + step, hi - step, np.nextafter(hi, F32(0)), hi, np.nextafter(hi, one), hi + step]

    rows = sorted({guard["row_lo"] - 1, guard["row_lo"], guard["row_hi"], guard["row_hi"] + 1})
    inside = (rx // 2, ry // 2, F32(0.5), F32(0.5))
    outside = (rx // 2, 0, F32(0.0), F32(1.0) - F32(2.0 ** -24))
    cases = []
    for base in (inside, outside):
        for r in around(du):
            cases.append((base[0], base[1], r, base[3]))
        for r in around(dv):
            cases.append((base[0], base[1], base[2], r))
        for row in rows:
            cases.append((base[0], row, base[2], base[3]))
    for col in (0, rx - 1):  # the seam
        for r in around(du):
            cases.append((col, ry // 2, r, F32(0.5)))
    return cases


@pytest.mark.parametrize("res", TABLES)
def test_draws_on_both_sides_of_every_bound_in_every_kind_of_wave(hb, tables, res):
    rx, ry = res
    g = tables[res]
    _, _, guard = hb.selftest_sky_cell(g, [[0, 0, bits(0.5), bits(0.5)]])
    cases = _bound_cases(rx, ry, guard)
    inside, outside = (rx // 2, ry // 2, F32(0.5), F32(0.5)), (rx // 3, 0, F32(0.25), F32(0.75))
    words = []
    # waves of 64 consecutive cases: one all guarded, one all unguarded, then every bound case alone in a guarded wave, alone in an
    # unguarded wave, and the bound cases together (mixed)
    words += [inside] * 64 + [outside] * 64
    for c in cases:
        words += [c] + [inside] * 63
        words += [outside] * 63 + [c]
    words += (cases * (64 // len(cases) + 1))[:64 * ((len(cases) + 63) // 64)]
    arr = np.array([[c[0], c[1], bits(c[2]), bits(c[3])] for c in words], dtype=np.uint32)
    out, counts, _ = hb.selftest_sky_cell(g, arr)
    assert counts["tested"] == len(words)
    assert counts["guarded_disagree"] == 0 and counts["pdf_mismatches"] == 0, counts
    assert np.array_equal(out[:, 0], out[:, 1]), "the carried pdf differs from the default's"
    differ = np.flatnonzero((out[:, 2] & 0x7FFFFFFF) != out[:, 3])
    assert differ.size == 0, ("the cell the carried pdf was read at is not the default's", [(int(k), words[k], hex(int(out[k, 2])), hex(int(out[k, 3]))) for k in differ[:8]])
    guarded = (out[:, 2] >> 31).astype(bool)
    assert guarded[:64].all() and not guarded[64:128].any()
    # the guard bit is the stated rule, exactly: |r - 0.5| <= 0.5 - delta in f32 (rt_types.h DevSkyCell), which for a jitter a stream can
    # draw -- a multiple of 2^-24 -- is delta <= r <= 1 - delta
    du, dv, half, lattice = F32(guard["delta_u"]), F32(guard["delta_v"]), F32(0.5), 2.0 ** 24
    for k, (su, sv, ru, rv) in enumerate(words):
        want = bool(abs(F32(ru - half)) <= half - du and abs(F32(rv - half)) <= half - dv and guard["row_lo"] <= sv <= guard["row_hi"])
        assert bool(guarded[k]) == want, (k, su, sv, float(ru), float(rv))
        if float(ru) * lattice == int(float(ru) * lattice) and float(rv) * lattice == int(float(rv) * lattice):
            assert want == bool(du <= ru <= F32(1.0) - du and dv <= rv <= F32(1.0) - dv and guard["row_lo"] <= sv <= guard["row_hi"]), (k, su, sv)
    # with the switch off no lane is guarded and the pdfs are still the default's
    g.set_tuning(abi.RT_TUNE_SKY_CELL, 0)
    try:
        off, counts_off, guard_off = hb.selftest_sky_cell(g, arr)
    finally:
        g.set_tuning(abi.RT_TUNE_SKY_CELL, -1)
    assert guard_off["proven"] and not guard_off["enabled"]
    assert counts_off["unguarded"] == len(words) and counts_off["pdf_mismatches"] == 0
    assert np.array_equal(off[:, 0], out[:, 0])


def _frames(hb, scene, camera_params, split):
    """(frame, rays) with the switch on, off, and through the general spheres-only kernels"""
    cam = hb.camera_new(**camera_params)
    opts = abi.default_render_opts(64, 64, 16, method=abi.RT_METHOD_MIS, seed=5)
    opts.sample_split = split
    got = {}
    for label, key, value in (("on", abi.RT_TUNE_SKY_CELL, 1), ("off", abi.RT_TUNE_SKY_CELL, 0), ("general", abi.RT_TUNE_FEATURE_SET, 0)):
        g = hb.HipScene(scene, device=0)
        g.set_tuning(key, value)
        got[label] = g.render(cam, opts)
        assert g.last_launch_info()["feature_set"] == (0 if label == "general" else 3), (label, g.last_launch_info())
    return got, opts


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("name", ["rtweekend1", "two_spheres_7x5"])
def test_frames_do_not_depend_on_the_switch_and_are_the_oracles(hb, O, name, split):
    if name == "rtweekend1":
        ls = scenes.load_ssml("rtweekend1")
        scene, camera_params = ls.scene, ls.camera_params
    else:
        scene, camera_params = two_spheres((7, 5)), TWO_SPHERE_CAMERA
    got, opts = _frames(hb, scene, camera_params, split)
    ref, ref_rays = O.Scene(scene).render(O.camera_new(**camera_params), opts)
    for label, (img, rays) in got.items():
        assert_same_bits(img, got["on"][0], f"{name} split={split} {label} against on", nan_equal=True)
        assert rays == got["on"][1], (name, split, label, rays, got["on"][1])
    assert_same_bits(got["on"][0], ref, f"{name} split={split} against the oracle", nan_equal=True)
    assert got["on"][1] == ref_rays


@pytest.mark.parametrize("res", [(0, 0), (1, 1)])
def test_a_sky_the_host_must_refuse_keeps_the_flag_off(hb, res):
    scene = two_spheres(res)
    g = hb.HipScene(scene, device=0)
    if res != (0, 0):
        _, counts, guard = hb.selftest_sky_cell(g, [[0, 0, bits(0.5), bits(0.5)]] * 64)
        assert not guard["proven"] and not guard["enabled"]
        assert counts["unguarded"] == 64 and counts["pdf_mismatches"] == 0
    else:
        with pytest.raises(hb.RtHipError):
            hb.selftest_sky_cell(g, [[0, 0, bits(0.5), bits(0.5)]])
        guard = hb.sky_cell_guard(g)  # (answered without a launch, for any scene)
        assert not guard["proven"] and not guard["enabled"]
    cam = hb.camera_new(**TWO_SPHERE_CAMERA)
    opts = abi.default_render_opts(64, 64, 16, method=abi.RT_METHOD_MIS, seed=5)
    g.set_tuning(abi.RT_TUNE_SKY_CELL, 1)  # asking does not turn on what is not proven
    assert not hb.sky_cell_guard(g)["enabled"]
    on, rays_on = g.render(cam, opts)
    g.set_tuning(abi.RT_TUNE_SKY_CELL, 0)
    off, rays_off = g.render(cam, opts)
    assert_same_bits(on, off, f"sampler_res {res}", nan_equal=True)
    assert rays_on == rays_off
