"""raytracing-rust_amd/csrc/rt_lean.h, host pass of the short reciprocal / square-root forms.  On the host these forms are the plain
operators -- the device's are built from v_rcp_f32 / v_sqrt_f32 and are enumerated ON the GPU (rt_selftest_short_forms,
tests/test_gpu_short_forms.py) -- so this checks only that the translation units still compile for the host and that the host
statements agree with `1.0f / d` and `sqrtf` on the CPU.  It proves nothing about the device's instructions."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_host_statements_are_the_plain_operators(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "short_forms_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "short_forms_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout
    res = {name: (int(n), int(bad)) for name, n, bad in (line.split() for line in out.splitlines())}
    assert set(res) == {"lean_inv", "lean_inv_gfx950", "lean_sqrt"}
    for name, (n, bad) in res.items():
        assert n > 1000000 and bad == 0, (name, n, bad)
