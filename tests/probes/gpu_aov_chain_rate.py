"""Cost of the specular-chain AOV pass (rt_render_aov_chain_device) next to the first-hit pass (rt_render_aov_device) on the same
scene, frame and passes, timed with HIP events on one stream after a warm-up (as gpu_aov_rate.py): rtweekend1.ssml (no followed
surface: the ratio is the price of the loop shape), all_materials, the quality scene of tests/test_gpu_aov_chain.py and a
1 M-triangle random mesh, 1920 x 1080 x 16.
  python tests/probes/gpu_aov_chain_rate.py [--reps N]
Prints one JSON line per scene: ms (median of N) of both passes, their ratio and the mean `bounces`."""
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
import gpu_support as T  # noqa: E402  (the quality scene)

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
    cases = [("rtweekend1", ls.scene, ls.camera_params), ("all_materials", scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
             ("quality_scene", T.quality_scene(), T.QUALITY_CAMERA),
             ("mesh1m", scenes.random_triangle_mesh(1_000_000), scenes.MESH_CAMERA)]
    aov = {name: torch.zeros(W * H * (3 if name in ("albedo", "normal") else 1), dtype=torch.float32, device=dev)
           for name in abi.AOV_CHAIN_CHANNELS}
    chain_ptrs = {name: t.data_ptr() for name, t in aov.items()}
    first_ptrs = {name: chain_ptrs[name] for name in abi.AOV_CHANNELS}
    for name, sc, cam_params in cases:
        g = hb.HipScene(sc, device=0)
        cam = hb.camera_new(**cam_params)
        opts = abi.default_render_opts(W, H, SPP, seed=1)
        first_ms = timed(stream, lambda: g.render_aov_device(cam, opts, first_ptrs, stream=stream.cuda_stream))
        chain_ms = timed(stream, lambda: g.render_aov_chain_device(cam, opts, chain_ptrs, stream=stream.cuda_stream))
        bounces = float(aov["bounces"].mean().item())
        print(json.dumps({"scene": name, "size": f"{W}x{H}x{SPP}", "first_hit_ms": round(first_ms, 3), "chain_ms": round(chain_ms, 3),
                          "chain_over_first_hit": round(chain_ms / first_ms, 3), "mean_bounces": round(bounces, 4),
                          "one_plus_mean_bounces": round(1.0 + bounces, 4), "max_chain": 8, "fuzz_limit": 0.0,
                          "reps": REPS, "source_hash": bench.source_hash()}), flush=True)


if __name__ == "__main__":
    main()
