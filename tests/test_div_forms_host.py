"""The one-pair f32 quotient of raytracing-rust_amd/csrc/rt_lean.h (lean_div_core_gfx950) as a sequence of IEEE operations on the CPU:
with r = RN(1 / d), q0 = n * r, e = fma(-d, q0, n), q = fma(e, r, q0) against `n / d` over the 64 denominator significands the GPU
test enumerates x all 2^23 numerator significands, and over 10^7 seeded random significand pairs (tests/cpp/div_forms_check.cpp).
A stand-alone program, built with AddressSanitizer and UBSan.  That gfx950's refined reciprocal IS RN(1 / d), and that the device's
instructions return the same, is what tests/test_gpu_div_forms.py enumerates on the GPU."""
import div_forms_cases
import host_check

DENOMINATORS = [int(x) for x in div_forms_cases.DENOMINATORS]  # the list the GPU test enumerates


def test_the_one_pair_sequence_is_the_quotient_on_the_host(tmp_path):
    exe = host_check.build("div_forms_check", tmp_path, sanitize=True, extra=())
    res = host_check.run(exe, *(f"{d:x}" for d in DENOMINATORS), timeout=600)
    print(res)
    assert set(res) == {"listed", "random"}
    n, bad, bad_q0 = res["listed"]
    assert n == len(DENOMINATORS) << 23 and len(DENOMINATORS) == 64 and bad == 0, res
    assert bad_q0 > n // 100, res  # the check discriminates: without the correction pair many quotients differ
    n, bad, bad_q0 = res["random"]
    assert n == 10_000_000 and bad == 0 and bad_q0 > n // 100, res
