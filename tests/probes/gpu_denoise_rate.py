"""Cost of the A-Trous denoiser (rt_denoise_device, 5 iterations, all guides + variance) next to the render (rt_render_device)
and the AOV pass (rt_render_aov_device) at the same passes, timed with HIP events on one stream after a warm-up:
rtweekend1.ssml and a 1 M-triangle random mesh, 1920 x 1080 x 16.
  python tests/probes/gpu_denoise_rate.py [--reps N]
Prints one JSON line per scene: ms (median of N), the compulsory bytes per iteration W*H*(16 + 16 + 16) (read colour+variance, read
guide, write) and the rate they imply.  At 1080p the 100 MB working set lives in the 256 MiB Infinity Cache, so that rate is a
memory-side figure, not an HBM fraction.  Per-kernel times: run this under rocprofv3 --kernel-trace --stats in a run of its own."""
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

W, H, SPP, ITER = 1920, 1080, 16, 5
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7


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
    n = W * H
    rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    aov = {k: torch.zeros(n * (3 if k != "depth" else 1), dtype=torch.float32, device=dev) for k in ("albedo", "normal", "depth")}
    variance = torch.zeros(n, dtype=torch.float32, device=dev)
    dopts = hb.denoise_opts(W, H, iterations=ITER)
    ws = torch.empty(hb.denoise_workspace_bytes(dopts), dtype=torch.uint8, device=dev)
    out = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    for name, sc, cam_params in cases:
        g = hb.HipScene(sc, device=0)
        cam = hb.camera_new(**cam_params)
        o = abi.default_render_opts(W, H, SPP, method=abi.RT_METHOD_MIS, seed=1)
        o.sample_split = 0
        render_ms = timed(stream, lambda: g.render_device(cam, o, rgb.data_ptr(), stream=stream.cuda_stream))
        aov_ms = timed(stream, lambda: g.render_aov_device(cam, o, {k: v.data_ptr() for k, v in aov.items()}, stream=stream.cuda_stream))
        # a real variance: the squared luminance difference of two half renders (what rt_render_denoised feeds the filter)
        half = abi.default_render_opts(W, H, SPP // 2, method=abi.RT_METHOD_MIS, seed=1)
        a, _ = g.render(cam, half)
        half.sample_begin = SPP // 2
        b, _ = g.render(cam, half)
        import denoise_checker as K
        variance.copy_(torch.from_numpy(K.halves_variance(a, b, aov["albedo"].cpu().numpy().reshape(H, W, 3)).ravel()))
        ptrs = {"color": rgb.data_ptr(), "variance": variance.data_ptr(), **{k: v.data_ptr() for k, v in aov.items()}}
        dn_ms = timed(stream, lambda: g.denoise_device(ptrs, ws.data_ptr(), out.data_ptr(), dopts, stream=stream.cuda_stream))
        ptrs_nv = {k: v for k, v in ptrs.items() if k != "variance"}
        dn_nv_ms = timed(stream, lambda: g.denoise_device(ptrs_nv, ws.data_ptr(), out.data_ptr(), dopts, stream=stream.cuda_stream))
        bytes_per_iter = n * (16 + 16 + 16)
        print(json.dumps({"scene": name, "size": f"{W}x{H}x{SPP}", "iterations": ITER,
                          "denoise_ms": round(dn_ms, 4), "denoise_spatial_variance_ms": round(dn_nv_ms, 4),
                          "render_mis_ms": round(render_ms, 3), "aov_ms": round(aov_ms, 3),
                          "denoise_over_render": round(dn_ms / render_ms, 4),
                          "compulsory_bytes_per_iteration": bytes_per_iter,
                          "compulsory_GBps": round(bytes_per_iter * ITER / (dn_ms * 1e-3) / 1e9, 1),
                          "reps": REPS, "source_hash": bench.source_hash()}), flush=True)


if __name__ == "__main__":
    main()
