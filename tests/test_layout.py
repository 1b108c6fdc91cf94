"""raytracing-rust_amd/csrc/rt_layout.h, the carver every scene-owned post-processing buffer is laid out by: tests/cpp/layout_check.cpp
(a stand-alone host program, no HIP) built with the address and undefined-behaviour sanitizers and run: alignment, order,
disjointness, absent parts, the total at 2^31 pixels against 128-bit arithmetic, and a description beyond the fixed capacity."""
import os

import pytest

import host_check


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    if not os.path.exists(host_check.HIPCC):
        pytest.skip("hipcc not available")
    # host code only: the sanitizers go to the host side of the hipcc line (-Xarch_host), nothing is built for a GPU
    return host_check.build("layout_check", tmp_path_factory.mktemp("layout"), extra=("-O1", "-g", "-Wall", "-Werror"),
                            sanitize=("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"))


def test_layouts_are_aligned_ordered_disjoint_and_do_not_wrap(layout_check):
    res = host_check.run(layout_check, timeout=120)  # (a non-zero exit fails there, with the program's output)
    assert set(res) == {"ok"} and len(res["ok"]) == 1 and res["ok"][0] > 500, res
