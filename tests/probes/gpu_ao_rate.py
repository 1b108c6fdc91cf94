"""Cost of the ambient-occlusion pass (rt_render_ao_device) next to the first-hit AOV pass with only its depth channel
(rt_render_aov_device) over the same window -- one closest-hit walk per pass, the yardstick -- on rtweekend1.ssml, all_materials
and a 1 M-triangle random mesh, 1920 x 1080 x 16: K = 4 and K = 1 AO rays per pass, without a limit and with a radius of about 1 % of
the extent of what the camera sees.  HIP events on one stream, the median of N after a warm-up, the two passes interleaved call by
call in one process.  Beside the ratio stands 1 + K * coverage, the number of walks per pass relative to the yardstick's one.
  python tests/probes/gpu_ao_rate.py [--reps N] [--scenes rtweekend1,all_materials,mesh1m] [--rays 4,1]
RT_HIP_LIB selects another build of the library (the A/B builds of the ballot quorum, -DRT_AO_QUORUM=n).
Prints one JSON line per scene, K and radius."""
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


def _arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


REPS = int(_arg("--reps", "7"))
# about 1 % of the extent of what the camera sees (the ground spheres, 100 and 1000 units, left out): the ball and its surroundings
# on rtweekend1, the row of balls of all_materials, the 20-unit cube of the mesh
RADIUS = {"rtweekend1": 0.05, "all_materials": 0.06, "mesh1m": 0.2}


def timed_interleaved(stream, fns):
    """median ms of REPS calls of each fn() on `stream` (HIP events around each call) after two warm-up calls each; the calls of
    one repetition follow each other, so that every fn sees the same machine"""
    for _ in range(2):
        for fn in fns:
            fn()
    stream.synchronize()
    ms = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [float(np.median(m)) for m in ms]


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    wanted = _arg("--scenes", "rtweekend1,all_materials,mesh1m").split(",")
    rays = [int(k) for k in _arg("--rays", "4,1").split(",")]
    n = W * H
    depth = torch.zeros(n, dtype=torch.float32, device=dev)
    coverage = torch.zeros(n, dtype=torch.float32, device=dev)
    vis = torch.zeros(n, dtype=torch.float32, device=dev)
    bent = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    ao_ptrs = {"visibility": vis.data_ptr(), "bent_normal": bent.data_ptr()}
    for name in wanted:
        if name == "rtweekend1":
            ls = scenes.load_ssml("rtweekend1")
            sc, cam_params = ls.scene, ls.camera_params
        elif name == "all_materials":
            sc, cam_params = scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA
        else:
            sc, cam_params = scenes.random_triangle_mesh(1_000_000), scenes.MESH_CAMERA
        g = hb.HipScene(sc, device=0)
        cam = hb.camera_new(**cam_params)
        opts = abi.default_render_opts(W, H, SPP, seed=1)
        with torch.cuda.stream(stream):
            g.render_aov_device(cam, opts, {"coverage": coverage.data_ptr()}, stream=stream.cuda_stream)
            stream.synchronize()
            cover = float(coverage.mean().item())
            for k in rays:
                for radius in (0.0, RADIUS[name]):
                    first_ms, ao_ms = timed_interleaved(stream, [
                        lambda: g.render_aov_device(cam, opts, {"depth": depth.data_ptr()}, stream=stream.cuda_stream),
                        lambda: g.render_ao_device(cam, opts, ao_ptrs, rays_per_pass=k, radius=radius, stream=stream.cuda_stream)])
                    stream.synchronize()
                    print(json.dumps({"scene": name, "size": f"{W}x{H}x{SPP}", "rays_per_pass": k, "radius": radius,
                                      "first_hit_depth_ms": round(first_ms, 3), "ao_ms": round(ao_ms, 3),
                                      "ao_over_first_hit": round(ao_ms / first_ms, 3), "coverage": round(cover, 4),
                                      "one_plus_k_coverage": round(1.0 + k * cover, 3),
                                      "mean_visibility": round(float(vis.mean().item()), 4),
                                      "ao_rays_per_s": round(n * SPP * k * cover / (ao_ms * 1e-3)),
                                      "lib": os.path.basename(hb.LIB_PATH), "reps": REPS, "source_hash": bench.source_hash()}),
                          flush=True)


if __name__ == "__main__":
    main()
