"""The argument checks of the case-table self-tests (rt_selftest_pair_shadow, _pair_shadow_walk, _frame_forms, _gen_keys and the
operand modes of rt_selftest_short_forms and rt_selftest_div_forms) come BEFORE the device is looked at: no cases, one case past the
limit, a NULL out pointer -- and for rt_selftest_div_forms a slice next to operands -- are RT_ERR_INVALID_ARGUMENT even on a device
ordinal nothing has, where the same calls with valid arguments are RT_ERR_NO_DEVICE.  The library loads without a GPU, as
tests/test_gen_keys_host.py relies on; nothing here reaches one."""
import ctypes as C

import numpy as np
import pytest

NO_SUCH_DEVICE = 99  # past any machine's ordinals: with valid arguments every call below ends at the device check, GPU or none


def _pf(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def _case_table(symbol, width, n_counts, dtype=np.float32, ctype=C.c_float, lead=()):
    """call(cases, n, out) of an rt_selftest_*(device, [seed,] cases, n_cases, counts) entry point"""
    def call(lib, cases, n, out):
        return getattr(lib, symbol)(C.c_int(NO_SUCH_DEVICE), *lead, _pf(cases, ctype), C.c_uint64(n), out)
    return call, width, dtype, (C.c_uint64 * n_counts)(), 1 << 22


def _short_forms(abi):
    res = abi.ShortFormsResult()

    def call(lib, ops, n, out):
        return lib.rt_selftest_short_forms(C.c_int(NO_SUCH_DEVICE), _pf(ops), C.c_uint64(n), out)
    return call, 1, np.float32, C.byref(res), 1 << 20


def _div_forms(abi):
    res = abi.DivFormsResult()

    def call(lib, pairs, n, out):
        return lib.rt_selftest_div_forms(C.c_int(NO_SUCH_DEVICE), None, _pf(pairs), C.c_uint64(n), out)
    return call, 2, np.float32, C.byref(res), 1 << 20


SELFTESTS = {
    "pair_shadow": lambda abi: _case_table("rt_selftest_pair_shadow", abi.PAIR_SHADOW_CASE_FLOATS, len(abi.PAIR_SHADOW_COUNT_NAMES)),
    "pair_shadow_walk": lambda abi: _case_table("rt_selftest_pair_shadow_walk", abi.PAIR_SHADOW_WALK_CASE_FLOATS, len(abi.PAIR_SHADOW_WALK_COUNT_NAMES)),
    "frame_forms": lambda abi: _case_table("rt_selftest_frame_forms", 3, len(abi.FRAME_FORMS_COUNT_NAMES)),
    "gen_keys": lambda abi: _case_table("rt_selftest_gen_keys", abi.GEN_KEYS_CASE_WORDS, len(abi.GEN_KEYS_COUNT_NAMES), np.uint32, C.c_uint32,
                                        lead=(C.c_uint64(1),)),
    "short_forms": _short_forms,
    "div_forms": _div_forms,
}


@pytest.mark.parametrize("name", sorted(SELFTESTS))
def test_bad_arguments_are_refused_before_the_device_is_looked_at(hb, abi, name):
    lib = hb.lib()
    call, width, dtype, out, limit = SELFTESTS[name](abi)
    cases = np.zeros((limit + 1, width), dtype=dtype)  # (never touched: the pages stay unmapped)
    assert call(lib, cases, 0, out) == abi.RT_ERR_INVALID_ARGUMENT, "no cases"
    assert call(lib, cases, limit + 1, out) == abi.RT_ERR_INVALID_ARGUMENT, "one case past the limit"
    assert call(lib, cases, 1, None) == abi.RT_ERR_INVALID_ARGUMENT, "NULL out pointer"
    # the same calls with valid arguments get as far as the device, at either end of the range
    assert call(lib, cases, 1, out) == abi.RT_ERR_NO_DEVICE
    assert call(lib, cases, limit, out) == abi.RT_ERR_NO_DEVICE
    assert b"no such HIP device" in lib.rt_last_error()


def test_div_forms_takes_a_slice_or_operands_not_both(hb, abi):
    lib = hb.lib()
    res, pairs, exps = abi.DivFormsResult(), np.ones((1, 2), dtype=np.float32), np.zeros((1, 2), dtype=np.int32)
    sl = abi.DivFormsSlice()
    sl.denominators, sl.n_denominators, sl.first_denominator = None, 1, 0
    sl.exponents, sl.n_exponent_pairs = _pf(exps, C.c_int32), 1
    dev = C.c_int(NO_SUCH_DEVICE)
    assert lib.rt_selftest_div_forms(dev, C.byref(sl), _pf(pairs), C.c_uint64(1), C.byref(res)) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_selftest_div_forms(dev, None, None, C.c_uint64(0), C.byref(res)) == abi.RT_ERR_INVALID_ARGUMENT  # ... nor neither
    assert lib.rt_selftest_div_forms(dev, C.byref(sl), None, C.c_uint64(0), None) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_selftest_div_forms(dev, C.byref(sl), None, C.c_uint64(0), C.byref(res)) == abi.RT_ERR_NO_DEVICE
