"""Resource budget of the temporal accumulation kernels (csrc/rt_temporal.hip): no scratch, no spilled registers, a 256-thread
maximum workgroup and at least four waves per SIMD by registers (the kernels fit eight today: DESIGN.md section 11).  They are their
own translation unit, so their code object is an offload bundle of its own in librt_hip.so, found here as the denoiser's is
(tests/test_denoise_resources.py).  The denoiser's kernels are launched from it but never instantiated in it."""
import importlib.util
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tests", "probes", "resource_table.py"))
rtab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rtab)
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNELS = {"rt::temporal_reproject", "rt::temporal_resolve", "rt::temporal_feedback"}


@pytest.fixture(scope="module")
def temporal_bundle():
    """every kernel of the bundle that holds the temporal kernels"""
    if not os.path.exists(rtab.READELF):
        pytest.skip("llvm-readelf not available")
    csrc = os.path.join(ROOT, "raytracing-rust_amd", "csrc")
    srcs = [os.path.join(csrc, n) for n in os.listdir(csrc) if n.endswith((".hip", ".h", ".cpp")) or n == "Makefile"]
    if not os.path.exists(rtab.LIB) or os.path.getmtime(rtab.LIB) < max(os.path.getmtime(p) for p in srcs):
        subprocess.run(["make", "-C", csrc, "-s", "../librt_hip.so"], check=True)
    data = open(rtab.LIB, "rb").read()
    bundles = []
    i = data.find(MAGIC)
    while i >= 0:
        with tempfile.NamedTemporaryFile(suffix=".bundle") as f:
            f.write(data[i:])
            f.flush()
            bundles.append(rtab.extract(f.name))
        i = data.find(MAGIC, i + len(MAGIC))
    found = [b for b in bundles if any("temporal_" in k for k in b)]
    assert len(found) == 1, [sorted(b) for b in found]
    return found[0]


def test_temporal_kernel_resources(temporal_bundle):
    assert set(temporal_bundle) == KERNELS, sorted(temporal_bundle)
    for name, d in temporal_bundle.items():
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["waves_per_simd_by_registers"] >= 4, (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)


def test_no_render_aov_or_denoiser_kernel_in_the_temporal_bundle(temporal_bundle):
    assert not any(w in k for k in temporal_bundle for w in ("render_kernel", "aov_kernel", "denoise_")), sorted(temporal_bundle)
