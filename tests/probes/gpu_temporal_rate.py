"""Cost of one temporal step (rt_denoise_temporal_device with a history, 5 iterations, all guides) next to the spatial filter
alone (rt_denoise_device, same inputs, no variance: what the step does without history) and the render at the same passes, timed
with HIP events on one stream after a warm-up: rtweekend1.ssml, 1920 x 1080 x 16, a camera orbiting 0.5 degrees per step.
  python tests/probes/gpu_temporal_rate.py [--reps N]
Prints one JSON line: ms (median of N, default 9) and the compulsory bytes of the temporal part per pixel.  The steady state is timed:
each timed call reads the history the previous one wrote (two buffers, alternating).  Per-kernel times: run this under
rocprofv3 --kernel-trace --stats in a run of its own."""
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
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
# per pixel: colour + albedo + normal (36) + depth (4) read, plane1 + H0 + H1 + H2 written (64) and four taps of three history
# planes (48, once each when neighbours share them) by the reprojection; resolve reads plane0 + H0 (+ H2) and writes plane0 (48);
# the feedback reads plane1 + H0 and writes H0 (48): ~250 B, against 48 B per A-Trous iteration
TEMPORAL_BYTES_PER_PIXEL = 36 + 4 + 64 + 48 + 48 + 48


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
    g = hb.HipScene(ls.scene, device=0)
    p = ls.camera_params
    at, o = np.array(p["lookat"], np.float64), np.array(p["origin"], np.float64)

    def cam_at(i):
        t = np.radians(0.5 * i)
        r = o - at
        r = np.array([np.cos(t) * r[0] + np.sin(t) * r[2], r[1], -np.sin(t) * r[0] + np.cos(t) * r[2]])
        return hb.camera_new(**dict(p, origin=tuple(at + r)))

    cams = [cam_at(0), cam_at(1)]
    n = W * H
    rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    aov = {k: torch.zeros(n * (3 if k != "depth" else 1), dtype=torch.float32, device=dev) for k in ("albedo", "normal", "depth")}
    o16 = abi.default_render_opts(W, H, SPP, method=abi.RT_METHOD_MIS, seed=1)
    o16.sample_split = 0
    render_ms = timed(stream, lambda: g.render_device(cams[1], o16, rgb.data_ptr(), stream=stream.cuda_stream))
    g.render_aov_device(cams[1], o16, {k: v.data_ptr() for k, v in aov.items()}, stream=stream.cuda_stream)
    stream.synchronize()
    ptrs = {"color": rgb.data_ptr(), **{k: v.data_ptr() for k, v in aov.items()}}
    dopts = hb.denoise_opts(W, H, iterations=ITER)
    dws = torch.empty(hb.denoise_workspace_bytes(dopts), dtype=torch.uint8, device=dev)
    out = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    spatial_ms = timed(stream, lambda: g.denoise_device(ptrs, dws.data_ptr(), out.data_ptr(), dopts, stream=stream.cuda_stream))
    topts = hb.temporal_opts(W, H, iterations=ITER)
    hist = [torch.zeros(hb.temporal_history_bytes(topts), dtype=torch.uint8, device=dev) for _ in range(2)]
    tws = torch.empty(hb.temporal_workspace_bytes(topts), dtype=torch.uint8, device=dev)
    motion = torch.zeros(n * 2, dtype=torch.float32, device=dev)
    # the first frame (no history) into hist[0]; each timed step then alternates cameras and history buffers
    g.denoise_temporal_device(ptrs, cams[0], None, 0, hist[0].data_ptr(), tws.data_ptr(), out.data_ptr(), topts,
                              stream=stream.cuda_stream)
    state = {"k": 0}

    def step():
        k = state["k"]
        g.denoise_temporal_device(ptrs, cams[(k + 1) % 2], cams[k % 2], hist[k % 2].data_ptr(), hist[(k + 1) % 2].data_ptr(),
                                  tws.data_ptr(), out.data_ptr(), topts, d_motion=motion.data_ptr(), stream=stream.cuda_stream)
        state["k"] = k + 1

    temporal_ms = timed(stream, step)
    print(json.dumps({"scene": "rtweekend1", "size": f"{W}x{H}x{SPP}", "iterations": ITER,
                      "temporal_step_ms": round(temporal_ms, 4), "spatial_filter_ms": round(spatial_ms, 4),
                      "temporal_overhead_ms": round(temporal_ms - spatial_ms, 4), "render_mis_ms": round(render_ms, 3),
                      "estimate_ms": 1.3, "temporal_compulsory_bytes_per_pixel": TEMPORAL_BYTES_PER_PIXEL,
                      "reps": REPS, "source_hash": bench.source_hash()}), flush=True)


if __name__ == "__main__":
    main()
