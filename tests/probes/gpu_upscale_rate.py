"""Cost of AOV-guided upscaling (rt_upscale_device) 960 x 540 -> 1920 x 1080, timed with HIP events on one stream after a warm-up
(median of N), and the end-to-end frame it buys: render + AOV + filter at full size against render + AOV + filter at 960 x 540 plus
the full-size AOV pass plus the upscale, on rtweekend1.ssml and a 1 M-triangle random mesh, 16 MIS passes.
  python tests/probes/gpu_upscale_rate.py [--reps N] [--only-upscale]
Prints one JSON line per scene.  Compulsory bytes of the upscale with all guides: source w*h*(12 + 12 + 12 + 4), destination guides
W*H*(12 + 12 + 4), written W*H*12 (the stage map, W*H, is not asked for).  --only-upscale times nothing but the stage (for a run
under rocprofv3 --kernel-trace --stats, in a run of its own)."""
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

(w, h), (W, H), SPP = (960, 540), (1920, 1080), 16
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
ONLY = "--only-upscale" in sys.argv
GUIDES = ("albedo", "normal", "depth")


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
    sh = stream.cuda_stream
    ls = scenes.load_ssml("rtweekend1")
    cases = [("rtweekend1", lambda: ls.scene, ls.camera_params)]
    if not ONLY:
        cases.append(("mesh1m", lambda: scenes.random_triangle_mesh(1_000_000), scenes.MESH_CAMERA))
    f = lambda count: torch.zeros(count, dtype=torch.float32, device=dev)  # noqa: E731
    n, N = w * h, W * H
    small = dict(rgb=f(3 * n), clean=f(3 * n), **{k: f(n * (3 if k != "depth" else 1)) for k in GUIDES})
    full = dict(rgb=f(3 * N), clean=f(3 * N), **{k: f(N * (3 if k != "depth" else 1)) for k in GUIDES})
    out, stage = f(3 * N), torch.zeros(N, dtype=torch.uint8, device=dev)
    d_small, d_full = hb.denoise_opts(w, h), hb.denoise_opts(W, H)
    ws = torch.empty(hb.denoise_workspace_bytes(d_full), dtype=torch.uint8, device=dev)
    uopts = hb.upscale_opts(w, h, W, H)
    for name, make, cam_params in cases:
        g = hb.HipScene(make(), device=0)
        cam = hb.camera_new(**cam_params)

        def opts(ww, hh):
            o = abi.default_render_opts(ww, hh, SPP, method=abi.RT_METHOD_MIS, seed=1)
            o.sample_split = 0
            return o

        def render(buf, ww, hh):
            g.render_device(cam, opts(ww, hh), buf["rgb"].data_ptr(), stream=sh)

        def aov(buf, ww, hh):
            g.render_aov_device(cam, opts(ww, hh), {k: buf[k].data_ptr() for k in GUIDES}, stream=sh)

        def denoise(buf, dopts):
            g.denoise_device({"color": buf["rgb"].data_ptr(), **{k: buf[k].data_ptr() for k in GUIDES}}, ws.data_ptr(),
                             buf["clean"].data_ptr(), dopts, stream=sh)

        def upscale(guided=True, with_stage=False):
            ptrs = {"color": small["clean"].data_ptr()}
            if guided:
                ptrs.update({"src_" + k: small[k].data_ptr() for k in GUIDES})
                ptrs.update({"dst_" + k: full[k].data_ptr() for k in GUIDES})
            g.upscale_device(ptrs, out.data_ptr(), uopts, stage.data_ptr() if with_stage else 0, stream=sh)

        def small_frame():
            render(small, w, h)
            aov(small, w, h)
            denoise(small, d_small)
            aov(full, W, H)
            upscale()

        def full_frame():
            render(full, W, H)
            aov(full, W, H)
            denoise(full, d_full)

        small_frame()  # real inputs for the stage
        stream.synchronize()
        row = {"scene": name, "size": f"{w}x{h} -> {W}x{H}", "passes": SPP, "reps": REPS, "source_hash": bench.source_hash()}
        row["upscale_all_guides_ms"] = round(timed(stream, upscale), 4)
        row["upscale_no_guides_ms"] = round(timed(stream, lambda: upscale(guided=False)), 4)
        upscale(with_stage=True)
        stream.synchronize()
        share = np.bincount(stage.cpu().numpy(), minlength=4) / N
        row["stage_share_0_to_3"] = [round(float(v), 6) for v in share]
        compulsory = n * (12 + 12 + 12 + 4) + N * (12 + 12 + 4) + N * 12
        row["compulsory_bytes"] = compulsory
        row["compulsory_GBps"] = round(compulsory / (row["upscale_all_guides_ms"] * 1e-3) / 1e9, 1)
        if not ONLY:
            row["render_small_ms"] = round(timed(stream, lambda: render(small, w, h)), 3)
            row["aov_small_ms"] = round(timed(stream, lambda: aov(small, w, h)), 3)
            row["denoise_small_ms"] = round(timed(stream, lambda: denoise(small, d_small)), 4)
            row["render_full_ms"] = round(timed(stream, lambda: render(full, W, H)), 3)
            row["aov_full_ms"] = round(timed(stream, lambda: aov(full, W, H)), 3)
            row["denoise_full_ms"] = round(timed(stream, lambda: denoise(full, d_full)), 4)
            row["frame_small_upscaled_ms"] = round(timed(stream, small_frame), 3)
            row["frame_full_ms"] = round(timed(stream, full_frame), 3)
            row["full_over_upscaled"] = round(row["frame_full_ms"] / row["frame_small_upscaled_ms"], 3)
        print(json.dumps(row), flush=True)
        g.close()


if __name__ == "__main__":
    main()
