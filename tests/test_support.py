"""The shared test helpers themselves (tests/gpu_support.py, tests/resource_budget.py), without a GPU: what assert_same_bits lets
through and what it does not, the layout and the guard checks of GuardedBuffers on CPU tensors, and each condition of
assert_budget on hand-made tables."""
import numpy as np
import pytest

from gpu_support import GuardedBuffers, assert_same_bits
from resource_budget import assert_budget

F32 = np.float32
Failed = pytest.fail.Exception


def _f32(*words):
    return np.array(words, np.uint32).view(F32)


# ---- assert_same_bits ----
@pytest.mark.parametrize("nan_equal", [True, False])
def test_same_bits_passes_on_identical_arrays(nan_equal):
    a = np.array([[0.0, -0.0, 1.5], [np.inf, np.nan, -2.0]], F32)
    assert_same_bits(a, a.copy(), "identical", nan_equal=nan_equal)
    assert_same_bits(np.zeros((0, 3), F32), np.zeros((0, 3), F32), "empty", nan_equal=nan_equal)


@pytest.mark.parametrize("nan_equal", [True, False])
def test_same_bits_fails_on_dtype_shape_sign_of_zero_one_ulp_and_nan_against_a_number(nan_equal):
    one = np.ones((2, 3), F32)
    with pytest.raises(AssertionError, match="float64"):  # both dtypes are reported
        assert_same_bits(one, one.astype(np.float64), "dtype", nan_equal=nan_equal)
    with pytest.raises(AssertionError, match=r"\(3, 2\)"):  # and both shapes
        assert_same_bits(one, one.reshape(3, 2), "shape", nan_equal=nan_equal)
    for what, other in (("zero", -0.0), ("ulp", np.nextafter(F32(1.0), F32(2.0))), ("nan", np.nan)):
        a, b = one.copy(), one.copy()
        a[1, 2], b[1, 2] = (0.0 if what == "zero" else 1.0), other
        with pytest.raises(Failed, match=rf"{what}: 1 elements differ, first at \[1, 2\]: gpu .* checker "):
            assert_same_bits(a, b, what, nan_equal=nan_equal)


def test_same_bits_nan_payloads():
    quiet, payload = _f32(0x7FC00000, 0x3F800000), _f32(0x7FC0BEEF, 0x3F800000)
    assert np.isnan(quiet[0]) and np.isnan(payload[0])
    assert_same_bits(quiet, payload, "payloads", nan_equal=True)
    with pytest.raises(Failed, match="1 elements differ"):
        assert_same_bits(quiet, payload, "payloads", nan_equal=False)
    assert_same_bits(payload, payload.copy(), "the same payload", nan_equal=False)


@pytest.mark.parametrize("nan_equal", [True, False])
def test_same_bits_compares_integers_by_value(nan_equal):
    a = np.array([0, 7, 0x7FC0BEEF, 0xFFFFFFFF], np.uint32)
    assert_same_bits(a, a.copy(), "ids", nan_equal=nan_equal)
    b = a.copy()
    b[3] = 0xFFFFFFFE
    with pytest.raises(Failed, match=r"first at \[3\]"):
        assert_same_bits(a, b, "ids", nan_equal=nan_equal)


def test_same_bits_takes_scalars_through_asarray():
    """a float32 scalar against a 0-d float32 array compares; a Python float is float64 and fails on its dtype"""
    assert_same_bits(F32(0.25), np.asarray(0.25, F32), "scalar", nan_equal=True)
    with pytest.raises(Failed, match=r"first at \[\]"):
        assert_same_bits(F32(0.25), np.asarray(0.5, F32), "scalar", nan_equal=True)
    with pytest.raises(AssertionError, match="float64"):
        assert_same_bits(0.25, np.asarray(0.25, F32), "python float", nan_equal=True)


# ---- GuardedBuffers ----
SPEC = {"plane": ((3, 5), np.float32), "ids": ((2, 3, 5), np.uint32)}
DEFAULT_GUARD = 0x5A5A5A5A


@pytest.mark.parametrize("off", [0, 1, 3])
def test_guarded_buffers_on_cpu_tensors(off):
    import torch
    run = GuardedBuffers(torch, SPEC, off=off, device="cpu")
    body = {"plane": np.arange(15, dtype=F32).reshape(3, 5) - F32(4.5), "ids": np.arange(30, dtype=np.uint32).reshape(2, 3, 5)}
    assert set(run.ptrs()) == set(SPEC) and set(run.ptrs(("ids",))) == {"ids"}
    for name, (shape, dtype) in SPEC.items():
        n, lo = int(np.prod(shape)), 4 + off
        words = run.buf[name].numpy().view(np.uint32)  # shares the tensor's memory

        def write_body():
            words[lo:lo + n] = body[name].reshape(-1).view(np.uint32)

        assert run.ptr(name) - run.buf[name].data_ptr() == 4 * (4 + off) and run.ptrs()[name] == run.ptr(name)
        assert len(words) - (lo + n) >= 4  # at least four guard words behind the body
        assert run.untouched(name)
        assert (run.read(name).view(np.uint32) == DEFAULT_GUARD).all()  # an unwritten body reads as the guard, in dtype and shape
        write_body()
        got = run.read(name)
        assert got.dtype == dtype and got.shape == shape and got.tobytes() == body[name].tobytes()
        assert not run.untouched(name)
        for index in (lo - 1, 0, lo + n, len(words) - 1):  # one word before the body, one after it
            words[index] = 1
            with pytest.raises(AssertionError, match=f"{name}: a guard value was overwritten"):
                run.read(name)
            words[index] = DEFAULT_GUARD
        run.read(name)
        # a partial read: the first `used` words are the output, the rest of the body must still hold the guard
        run.refill()
        assert run.untouched(name)
        used = n // shape[0]
        words[lo:lo + used] = body[name].reshape(-1).view(np.uint32)[:used]
        part = run.read(name, used=used)
        assert part.dtype == dtype and part.shape == (1,) + shape[1:] and part.tobytes() == body[name][:1].tobytes()
        words[lo + used] = 1
        with pytest.raises(AssertionError, match=f"{name}: a guard value was overwritten"):
            run.read(name, used=used)
        run.read(name)  # (the whole body may hold anything)
    for name in SPEC:  # (refill() above cleared every channel)
        run.buf[name].numpy().view(np.uint32)[4 + off:4 + off + body[name].size] = body[name].reshape(-1).view(np.uint32)
    assert {k: v.tobytes() for k, v in run.read_all().items()} == {k: v.tobytes() for k, v in body.items()}
    assert set(run.read_all(("plane",))) == {"plane"}
    run.refill()
    assert all(run.untouched(name) for name in SPEC)


def test_guarded_buffers_take_another_guard_value():
    import torch
    run = GuardedBuffers(torch, {"ids": ((2, 4), np.uint32)}, guard=0x7FC0BEEF, device="cpu")
    words = run.buf["ids"].numpy().view(np.uint32)
    assert (words == 0x7FC0BEEF).all() and run.untouched("ids")
    words[3] = DEFAULT_GUARD
    with pytest.raises(AssertionError, match="ids: a guard value was overwritten"):
        run.read("ids")


# ---- assert_budget ----
GOOD = dict(private_segment_fixed_size=0, vgpr_spill_count=0, sgpr_spill_count=0, waves_per_simd_by_registers=5,
            max_flat_workgroup_size=256, group_segment_fixed_size=8192)


def test_budget_passes_and_each_condition_fails_alone():
    assert_budget({"a": GOOD, "b": dict(GOOD, waves_per_simd_by_registers=8)}, waves=5)
    assert_budget({"a": GOOD}, waves=4, lds=8192)
    assert_budget({"a": dict(GOOD, max_flat_workgroup_size=1024)}, waves=4, workgroup=1024)
    for field, value, kw in (("private_segment_fixed_size", 16, {}), ("vgpr_spill_count", 1, {}), ("sgpr_spill_count", 1, {}),
                             ("waves_per_simd_by_registers", 4, {}), ("max_flat_workgroup_size", 1024, {}),
                             ("group_segment_fixed_size", 0, dict(lds=8192))):
        assert_budget({"a": GOOD}, waves=5, **kw)
        with pytest.raises(AssertionError, match="'b'"):  # the failure names the kernel
            assert_budget({"a": GOOD, "b": dict(GOOD, **{field: value})}, waves=5, **kw)
    with pytest.raises(AssertionError):
        assert_budget({}, waves=1)
