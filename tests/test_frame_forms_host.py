"""raytracing-rust_amd/csrc/rt_shade.h coord_from_z_pair -- the scatter frame as the two-sphere kernels form it: the arm chosen once by
selects on the operands, one guard, a literal zero component -- against the two-arm coord_from_z on the CPU, bit for bit (any NaN
equals any NaN): 10^6 seeded random unit normals and a grid of the edges (tests/cpp/frame_forms_check.cpp).  On the host the short
forms are the plain operators, so this proves the algebra of the rewrite; the device's instructions are compared by
tests/test_gpu_frame_forms.py.  A stand-alone program, its host code built with AddressSanitizer and UBSan."""
import host_check


def test_the_select_first_frame_is_the_two_arm_frame_on_the_host(tmp_path):
    res = host_check.run(host_check.build("frame_forms_check", tmp_path, sanitize=True), timeout=600)
    print(res)
    assert set(res) == {"random", "grid"}
    n, bad, passed, failed = res["random"]
    assert n == 1_000_000 and bad == 0, res
    assert failed < n // 1000, res  # a unit normal fails the guard only next to an axis or the equator: the cold copy stays cold
    n, bad, passed, failed = res["grid"]
    assert n == 32 ** 3 and bad == 0, res
    assert passed > 0 and failed > 0, res  # ... and the grid runs both sides of the guard
