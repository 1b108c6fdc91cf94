"""raytracing-rust_amd/csrc/rt_intersect.h sphere_occludes_unlimited -- what the two-sphere kernels ask of a sphere for a shadow ray
without a limit, answered from signs -- against Sphere::get_int's `hit && t > 0` on the CPU, where `/` and sqrtf are the arithmetic
contract's operators: 10^7 seeded random rays and spheres and a grid of the edges the proof names (tests/cpp/pair_shadow_check.cpp).
A stand-alone program, its host code built with AddressSanitizer and UBSan.  The device's instructions are compared by
tests/test_gpu_pair_shadow.py."""
import host_check


def test_the_sign_predicate_is_the_full_test_on_the_host(tmp_path):
    res = host_check.run(host_check.build("pair_shadow_check", tmp_path, sanitize=True), timeout=600)
    print(res)
    assert set(res) == {"random", "grid"}
    n, bad, bad_asked, asked = res["random"]
    assert n >= 10_000_000 and bad == 0 and bad_asked == 0, res
    assert asked < n // 100, res  # the cold path stays cold
    n, bad, bad_asked, asked = res["grid"]
    assert n > 10_000 and bad == 0 and bad_asked == 0, res
    assert asked > 0, res  # ... and the grid does reach it
