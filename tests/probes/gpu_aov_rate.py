"""Cost of the first-hit AOV pass (rt_render_aov_device) next to the render (rt_render_device) at the same passes, timed with
HIP events on one stream after a warm-up: rtweekend1.ssml and a 1 M-triangle random mesh, 1920 x 1080 x 16.
  python tests/probes/gpu_aov_rate.py [--reps N]
Prints one JSON line per scene and method: ms (median of N), primary rays/s and the AOV / render ratio."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("raytracing-rust_amd")
hb = importlib.import_module("raytracing-rust_amd.hip_backend")
abi = pkg.abi
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import scenes  # noqa: E402

W, H, SPP = 1920, 1080, 16
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5


def timed(stream, fn):
    """median ms of REPS calls of fn() on `stream` (HIP events around each call) after two warm-up calls"""
    for _ in range(2):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ls = scenes.load_ssml("rtweekend1")
    cases = [("rtweekend1", ls.scene, ls.camera_params), ("mesh1m", scenes.random_triangle_mesh(1_000_000), scenes.MESH_CAMERA)]
    rgb = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    aov = {name: torch.zeros(W * H * (3 if name in ("albedo", "normal") else 1), dtype=torch.float32, device=dev)
           for name in abi.AOV_CHANNELS}
    ptrs = {name: t.data_ptr() for name, t in aov.items()}
    for name, sc, cam_params in cases:
        g = hb.HipScene(sc, device=0)
        cam = hb.camera_new(**cam_params)
        aov_opts = abi.default_render_opts(W, H, SPP, seed=1)
        aov_ms = timed(stream, lambda: g.render_aov_device(cam, aov_opts, ptrs, stream=stream.cuda_stream))
        coverage = float(aov["coverage"].mean().item())
        for method in (abi.RT_METHOD_MIS, abi.RT_METHOD_NAIVE):
            o = abi.default_render_opts(W, H, SPP, method=method, seed=1)
            o.sample_split = 0
            render_ms = timed(stream, lambda: g.render_device(cam, o, rgb.data_ptr(), stream=stream.cuda_stream))
            print(json.dumps({"scene": name, "size": f"{W}x{H}x{SPP}", "method": "mis" if method else "naive",
                              "aov_ms": round(aov_ms, 3), "render_ms": round(render_ms, 3),
                              "aov_primary_rays_per_s": round(W * H * SPP / (aov_ms * 1e-3)),
                              "render_primary_rays_per_s": round(W * H * SPP / (render_ms * 1e-3)),
                              "aov_over_render": round(aov_ms / render_ms, 3), "coverage": round(coverage, 4),
                              "reps": REPS, "source_hash": bench.source_hash()}), flush=True)


if __name__ == "__main__":
    main()
