"""The sky's sampling tables as the host builds them (rt_scene_sky_info / rt_scene_get_sky_tables on host-only scenes), on every
case of tests/sky_cases.py: the CDFs against the oracle's word for word, the guide width against the rule restated here, every
guide entry against numpy's upper bound, the kernels' guided scan and the reference's binary search (transcribed in sky_cases.py)
against numpy on all 2^24 draws, the verified reciprocals against rt_selftest_division -- and that every case is in the regime
the table says it is in, reaches the cells it can reach, and that the tie cases really draw CDF entries.  No tolerance anywhere."""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import scenes
import sky_cases as SK
from gpu_support import assert_same_bits

abi = scenes.abi
F32 = np.float32
NAMES = list(SK.CASES)
GUIDED = [n for n in NAMES if SK.CASES[n].guide_k]
UNGUIDED_MONOTONE = [n for n in NAMES if not SK.CASES[n].guide_k and SK.CASES[n].monotone]


@functools.lru_cache(maxsize=None)
def _built(hb, O, name):
    """(sky info, rows, marginal, guide or None) of the host-only build and (rows, marginal) of the oracle, read-only"""
    sc = SK.sky_only(name)
    host = hb.HipScene(sc, device=abi.RT_DEVICE_NONE)
    info = host.sky_info()
    rows, marg, guide = host.sky_tables()
    rx, ry = SK.CASES[name].res
    o_rows, o_marg = O.Scene(sc).sky_tables(rx, ry)
    for a in (rows, marg, guide, o_rows, o_marg):
        if a is not None:
            a.setflags(write=False)
    return info, rows, marg, guide, o_rows, o_marg


def _monotone(cdf):
    return bool(np.isfinite(cdf).all() and (np.diff(cdf) >= 0).all())


@pytest.mark.parametrize("name", NAMES)
def test_tables_match_the_oracle(hb, O, name):
    info, rows, marg, _, o_rows, o_marg = _built(hb, O, name)
    assert (info["res_x"], info["res_y"]) == SK.CASES[name].res
    assert_same_bits(rows, o_rows, f"{name} row CDFs", nan_equal=True)
    assert_same_bits(marg, o_marg, f"{name} marginal CDF", nan_equal=True)


@pytest.mark.parametrize("name", NAMES)
def test_guide_width_follows_the_rule(hb, O, name):
    info, _, _, guide, o_rows, o_marg = _built(hb, O, name)
    rx, ry = SK.CASES[name].res
    usable = max(rx, ry) <= 254 and all(_monotone(c) for c in list(o_rows) + [o_marg])
    k = 0
    if usable:
        k = 16
        while k < max(rx, ry) and k < 256:
            k *= 2
    assert info["guide_k"] == k == SK.CASES[name].guide_k
    assert (guide is None) == (k == 0) and (guide is None or guide.shape == (ry + 1, k))
    assert SK.CASES[name].monotone == all(_monotone(c) for c in list(o_rows) + [o_marg])
    assert info["table_bytes"] == SK.table_bytes(rx, ry, k)


@pytest.mark.parametrize("name", GUIDED)
def test_guide_entries_are_upper_bounds(hb, O, name):
    info, _, _, guide, o_rows, o_marg = _built(hb, O, name)
    k = info["guide_k"]
    thresholds = (np.arange(k, dtype=np.float64) / k).astype(F32)  # exact
    for r, cdf in enumerate(list(o_rows) + [o_marg]):
        assert np.array_equal(guide[r], np.searchsorted(cdf, thresholds, side="right")), (name, r)


# ---- every possible draw ----
CHUNK = 1 << 21


def _over_all_draws(fn):
    """fn(draws) for the 2^24 draws in chunks, on a few threads (numpy releases the lock); returns the number of draws seen"""
    with ThreadPoolExecutor(max_workers=8) as pool:
        return sum(pool.map(lambda lo: fn(SK.all_draws(lo, lo + CHUNK)), range(0, 1 << 24, CHUNK)))


def _rows_to_search(name, rows, marg):
    out = {"marginal": (marg, len(rows)), "first row": (rows[0], 0)}
    if len(rows) > 1:  # (a table of one row: the last row is the first)
        out["last row"] = (rows[-1], len(rows) - 1)
    if name == "plateaus":
        zero = [r for r in range(len(rows)) if rows[r][-1] == 0.0]
        repeated = [r for r in range(len(rows)) if rows[r][-1] != 0.0 and (np.diff(rows[r]) == 0).any()]
        out["zero-sum row"] = (rows[zero[0]], zero[0])
        out["row with repeated entries"] = (rows[repeated[0]], repeated[0])
    return out


@pytest.mark.parametrize("name", GUIDED)
def test_three_searches_agree_on_every_draw(hb, O, name):
    _, _, _, guide, o_rows, o_marg = _built(hb, O, name)
    for what, (cdf, g) in _rows_to_search(name, o_rows, o_marg).items():
        def check(num):
            ref = SK.search_numpy(cdf, num)
            assert np.array_equal(SK.search_guided(cdf, guide[g], num), ref), (name, what, "guided scan")
            assert np.array_equal(SK.search_reference(cdf, num), ref), (name, what, "binary search")
            assert ref.min() >= 0 and ref.max() <= cdf.size - 2
            return num.size
        assert _over_all_draws(check) == 1 << 24


@pytest.mark.parametrize("name", UNGUIDED_MONOTONE)
def test_binary_search_is_the_upper_bound_on_every_draw(hb, O, name):
    _, _, _, guide, o_rows, o_marg = _built(hb, O, name)
    assert guide is None
    for what, (cdf, _) in _rows_to_search(name, o_rows, o_marg).items():
        def check(num):
            assert np.array_equal(SK.search_reference(cdf, num), SK.search_numpy(cdf, num)), (name, what)
            return num.size
        assert _over_all_draws(check) == 1 << 24


def test_binary_search_repeats_itself_without_an_order(hb, O):
    """`negative`: the CDF is not sorted, so there is no upper bound to compare with -- only the search's own determinism"""
    _, _, _, guide, o_rows, o_marg = _built(hb, O, "negative")
    assert guide is None
    for cdf in (o_marg, o_rows[0], o_rows[-1]):
        def check(num):
            a = SK.search_reference(cdf, num)
            assert np.array_equal(a, SK.search_reference(cdf, num.copy())) and a.min() >= 0 and a.max() <= cdf.size - 2
            return num.size
        assert _over_all_draws(check) == 1 << 24


# ---- the division u = nu / res_x ----
def _division(hb, divisor):
    rc, ok = C.c_float(), C.c_int()
    assert hb.lib().rt_selftest_division(C.c_float(divisor), C.byref(rc), C.byref(ok)) == 0
    return F32(rc.value), ok.value


@pytest.mark.parametrize("name", NAMES)
def test_reciprocals_are_those_of_the_division_selftest(hb, O, name):
    info = _built(hb, O, name)[0]
    rx, ry = SK.CASES[name].res
    if max(rx, ry) >= SK.VERIFIED_BELOW:
        # A DEPARTURE from the rule below, for the two huge cases only: the library runs no verification for a resolution of 2^24
        # or more (csrc/rt_api.cpp sky_reciprocals), reports inv_res_ok = 0 and stores no reciprocal -- although
        # rt_selftest_division, asked about that divisor, finds its reciprocal exact (asserted here, so that the reason for the
        # departure is checked).  What is compared is therefore the library's own range rule, not rt_selftest_division.
        assert _division(hb, float(max(rx, ry)))[1] == 1 and float(F32(max(rx, ry))) == max(rx, ry)
        assert name in SK.HUGE and info["inv_res_ok"] == 0 == SK.CASES[name].inv_res_ok
        assert_same_bits(np.array([info["inv_res_x"], info["inv_res_y"]], F32), np.zeros(2, F32), f"{name} reciprocals", nan_equal=False)
        return
    (rc_x, ok_x), (rc_y, ok_y) = _division(hb, float(rx)), _division(hb, float(ry))
    assert info["inv_res_ok"] == (1 if ok_x and ok_y else 0) == SK.CASES[name].inv_res_ok
    assert_same_bits(np.array([info["inv_res_x"], info["inv_res_y"]], F32), np.array([rc_x, rc_y], F32), f"{name} reciprocals", nan_equal=False)
    if ok_x:
        assert rc_x == F32(1.0) / F32(rx)


def test_both_forms_of_the_division_occur():
    """sky_sample's two forms of u = nu / res_x: the verified reciprocals on the 13 small tables, the plain division on the two of
    2^24 cells and more (no integer divisor from 1 to 6000 fails rt_selftest_division, nor does 2^24 - 1)"""
    ok = [c.inv_res_ok for c in SK.CASES.values()]
    assert ok.count(1) >= 2 and ok.count(0) >= 2


def test_no_small_resolution_takes_the_plain_division(hb):
    """why the plain-division cases are 64 MB tables: the host scan the table's rule asks for.  Every integer divisor from 1 to 300
    has a verified reciprocal, and so has 2^24 - 1, the one integer below 2^24 whose significand is all ones (the operand the
    two-fma correction is known to be weakest for); a scan to 6000 run by hand found none either.  So only the library's own
    range rule -- no verification from 2^24 on -- reaches the division."""
    unverified = [d for d in list(range(1, 301)) + [(1 << 24) - 1] if _division(hb, float(d))[1] != 1]
    assert unverified == []
    assert all(max(c.res) >= SK.VERIFIED_BELOW for c in SK.CASES.values() if not c.inv_res_ok)


def test_table_getter_checks_its_capacities(hb, O):
    host = hb.HipScene(SK.sky_only("control"), device=abi.RT_DEVICE_NONE)
    rows, marg, guide = np.zeros((8, 17), F32), np.zeros(9, F32), np.zeros((9, 16), np.uint8)
    get = hb.lib().rt_scene_get_sky_tables
    args = lambda nr, nm, ng: (host._h, rows.ctypes.data_as(C.c_void_p), C.c_uint64(nr), marg.ctypes.data_as(C.c_void_p), C.c_uint64(nm),
                               guide.ctypes.data_as(C.c_void_p), C.c_uint64(ng))
    for short in ((rows.size - 1, marg.size, guide.size), (rows.size, marg.size - 1, guide.size), (rows.size, marg.size, guide.size - 1)):
        assert get(*args(*short)) == abi.RT_ERR_INVALID_ARGUMENT
        assert not rows.any() and not marg.any() and not guide.any()  # nothing was written
    assert get(*args(rows.size, marg.size, guide.size)) == 0
    ref = _built(hb, O, "control")
    assert_same_bits(rows, ref[1], "rows", nan_equal=False)
    assert_same_bits(marg, ref[2], "marginal", nan_equal=False)
    assert np.array_equal(guide, ref[3])
    unsampled = hb.HipScene(SK.unsampled(SK.sky_only("control"), "control"), device=abi.RT_DEVICE_NONE)
    assert unsampled.sky_info()["table_bytes"] == 0
    assert get(unsampled._h, *args(rows.size, marg.size, guide.size)[1:]) == abi.RT_ERR_INVALID_ARGUMENT


# ---- every case says something ----
def test_every_case_is_in_its_regime(hb, O):
    for name, case in SK.CASES.items():
        info = _built(hb, O, name)[0]
        assert (info["table_bytes"] <= SK.LDS_LIMIT) == case.fits_lds == (name not in SK.BIG + SK.HUGE), name
    _, _, _, _, rows, marg = _built(hb, O, "plateaus")
    widths = np.diff(rows, axis=1)
    zero_rows = np.flatnonzero(rows[:, -1] == 0.0)
    assert len(zero_rows) >= 1 and (rows[zero_rows] == 0.0).all() and (np.diff(marg)[zero_rows] == 0.0).all()
    live = np.delete(widths, zero_rows, axis=0)
    no_pdf = (np.diff(marg)[:, None] * widths) == 0.0
    assert 0.28 < no_pdf.mean() < 0.40 and (live >= 0).all()  # about a third of the cells cannot be drawn
    assert (live == 0.0).any(axis=1).sum() >= 4 and (np.diff(marg) == 0.0).sum() == len(zero_rows)  # rows with repeated entries
    _, _, _, _, rows, marg = _built(hb, O, "negative")
    assert np.isfinite(marg).all() and (np.diff(marg) < 0).any() and (np.diff(marg) > 0).any()
    _, _, _, _, rows, marg = _built(hb, O, "black")
    assert not rows.view(np.uint32).any() and not marg.view(np.uint32).any()  # +0.0 everywhere
    for name in ("one_cell", "one_row", "one_column"):
        _, _, _, _, rows, marg = _built(hb, O, name)
        assert rows.shape == (SK.CASES[name].res[1], SK.CASES[name].res[0] + 1) and (rows[:, -1] == 1.0).all() and marg[-1] == 1.0


@functools.lru_cache(maxsize=None)
def _replayed(O, name, seed, n):
    """the cells (sv, su) the sampling reference's draws select in the oracle's tables, and which of the two searches of each
    stream drew a CDF entry exactly"""
    rx, ry = SK.CASES[name].res
    rows, marg = O.Scene(SK.sky_only(name)).sky_tables(rx, ry)
    draws = O.rng_streams_f32(seed, n, 4)  # marginal, row, then the two offsets inside the cell (sky.rs:64-78)
    sv = SK.search_numpy(marg, draws[:, 0])
    su = np.zeros(n, dtype=np.int64)
    tie_row = np.zeros(n, dtype=bool)
    for r in range(ry):
        mine = sv == r
        su[mine] = SK.search_numpy(rows[r], draws[mine, 1])
        tie_row[mine] = np.isin(draws[mine, 1], rows[r])
    return sv, su, np.isin(draws[:, 0], marg), tie_row, draws


@pytest.mark.parametrize("name", ("control", "plateaus") + SK.TIE_CASES)
def test_replay_is_the_oracles_sampling(O, name):
    """the replay above against the oracle's own sampler: the cells it finds and the third and fourth draw, carried through
    Sky::sample's arithmetic (sky.rs:64-78) with the oracle's next_float, sin and cos, give O.sample_directions bit for bit -- so
    the cell and tie counts of this file describe the streams the GPU self-test runs"""
    rx, ry = SK.CASES[name].res
    n = SK.SELFTEST_N
    sv, su, _, _, draws = _replayed(O, name, SK.SELFTEST_SEED, n)
    pi = F32(np.pi)  # RT_PI of include/rt_detmath.h
    u = O.utility(0, su.astype(F32) + draws[:, 2]) / F32(rx)
    v = O.utility(0, sv.astype(F32) + draws[:, 3]) / F32(ry)
    phi, theta = u * F32(2.0) * pi, v * pi
    st, ct, sp, cp = O.detmath(0, theta), O.detmath(1, theta), O.detmath(0, phi), O.detmath(1, phi)
    mine = np.stack([st * cp, st * sp, ct], axis=1)
    ref = O.Scene(SK.sky_only(name)).sample_directions(2, n, seed=SK.SELFTEST_SEED)
    assert mine.dtype == np.float32
    assert_same_bits(mine, ref, f"{name}: replayed directions", nan_equal=False)


@pytest.mark.parametrize("name", [n for n in NAMES if SK.CASES[n].monotone])
def test_selftest_draws_reach_the_cells(hb, O, name):
    """what the oracle's side of the GPU self-test covers: min(cells, 1000) distinct cells, or for the two cases whose tables rule
    that out what holds instead"""
    rx, ry = SK.CASES[name].res
    sv, su, _, _, _ = _replayed(O, name, SK.SELFTEST_SEED, SK.SELFTEST_N)
    cells = np.unique(sv * rx + su)
    if SK.CASES[name].one_cell_only:
        assert cells.tolist() == [rx * ry - 1]
        return
    _, _, _, _, rows, marg = _built(hb, O, name)
    wide = np.diff(marg)[:, None] * np.diff(rows, axis=1) > 0  # cells a draw can select
    # cells without width are never drawn (an upper bound steps over repeated entries); only `plateaus` and, by rounding, a
    # cell or two of the huge rows have any, so min(cells with width, 1000) is min(cells, 1000) everywhere else
    assert wide.ravel()[cells].all() and len(cells) >= min(int(wide.sum()), 1000)
    assert wide.all() or name == "plateaus" or (name in SK.HUGE and wide.sum() >= rx * ry - 2)


@pytest.mark.parametrize("name", SK.TIE_CASES)
def test_tie_cases_draw_cdf_entries(O, name):
    """`cdf[i] <= num` and `cdf[i] < num` part only where a draw equals an entry: at least 8 of the TIE_N streams do, per case"""
    _, _, tie_marginal, tie_row, _ = _replayed(O, name, SK.TIE_SEED, SK.TIE_N)
    ties = int(tie_marginal.sum() + tie_row.sum())
    print(f"{name}: {int(tie_marginal.sum())} marginal and {int(tie_row.sum())} row searches of {SK.TIE_N} streams draw a CDF entry")
    assert SK.TIE_N <= 1 << 22 and SK.TIE_N & (SK.TIE_N - 1) == 0
    assert ties >= 8
    assert (SK.CASES[name].guide_k != 0) == (name == SK.TIE_CASES[0])  # one guided, one unguided
