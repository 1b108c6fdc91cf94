"""Cost of the depth-of-field stage at 1920 x 1080.  HIP events on one stream, the median of REPS
repetitions after a warm-up, the calls interleaved:
    dof_focus_R     rt_dof_device at max_radius R = 4, 8, 16 over a frame wholly in focus (every radius 0.5: one tap per pixel)
    dof_scene_R     ... over the depth of scenes/rtweekend1.ssml (one AOV pass) with rt_dof_opts_from_camera at aperture 0.1
    dof_cap_R       ... with every radius clamped at R (everything at infinity, a huge blur_scale): (2R + 1)^2 taps per pixel
    copy            a device-to-device copy of the frame, for scale
    bloom           rt_bloom_device on the same frame (defaults)
    render_16spp    rt_render_device of the same scene, MIS, 16 passes: what the stage decorates
  python tests/probes/gpu_dof_rate.py [--reps N]
Prints one JSON line."""
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

W, H = 1920, 1080
RADII = (4, 8, 16)
APERTURE = 0.1


def _arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


REPS = int(_arg("--reps", "7"))
WARM = 2


def _timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    dev = torch.device("cuda", 0)
    n = W * H
    ls = scenes.load_ssml("rtweekend1")
    g = hb.HipScene(ls.scene, device=0)
    cam = hb.camera_new(**ls.camera_params)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    ropts = abi.default_render_opts(W, H, 16, method=abi.RT_METHOD_MIS, seed=1)
    frame, _ = g.render(cam, ropts)
    scene_depth = g.render_aov(cam, abi.default_render_opts(W, H, 1, seed=1), channels=("depth",))["depth"]
    focus = float(ls.camera_params["focus_dist"])
    rgb = torch.from_numpy(frame).to(dev)
    out = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    depths = {"focus": torch.full((n,), focus, dtype=torch.float32, device=dev), "scene": torch.from_numpy(scene_depth).to(dev),
              "cap": torch.zeros(n, dtype=torch.float32, device=dev)}
    ws = torch.zeros(hb.dof_workspace_bytes(hb.dof_opts(W, H)), dtype=torch.uint8, device=dev)
    calls, radii = {}, {}
    for R in RADII:
        opts = {"focus": hb.dof_opts(W, H, focus_distance=focus, blur_scale=8.0, max_radius=R, planar_depth=0),
                "scene": hb.dof_opts_from_camera(cam, APERTURE, focus, W, H, max_radius=R),
                "cap": hb.dof_opts(W, H, focus_distance=focus, blur_scale=1e6, max_radius=R, planar_depth=0)}
        for kind, o in opts.items():
            calls[f"dof_{kind}_{R}"] = (lambda o=o, kind=kind: g.dof_device(rgb.data_ptr(), depths[kind].data_ptr(), cam, o, ws.data_ptr(),
                                                                          out.data_ptr(), stream=s))
        radii[R] = round(float(opts["scene"].blur_scale), 4)
    bopts = hb.bloom_opts(W, H)
    bws = torch.zeros(hb.bloom_workspace_bytes(bopts), dtype=torch.uint8, device=dev)
    calls["bloom"] = lambda: g.bloom_device(rgb.data_ptr(), bopts, 0, bws.data_ptr(), out.data_ptr(), stream=s)
    calls["render_16spp"] = lambda: g.render_device(cam, ropts, out.data_ptr(), stream=s)

    def copy():
        with torch.cuda.stream(stream):
            out.copy_(rgb.view(-1))

    calls["copy"] = copy
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for rep in range(REPS + WARM):
        for k, fn in calls.items():
            t = _timed(stream, fn)
            if rep >= WARM:
                ms[k].append(t)
    print(json.dumps(dict(size=f"{W}x{H}", reps=REPS, warmup=WARM, lib=os.path.basename(hb.LIB_PATH), source_hash=bench.source_hash(),
                          aperture=APERTURE, blur_scale_of_the_scene=radii[RADII[0]],
                          sky_share_of_the_scene=round(float((scene_depth == 0).mean()), 4),
                          ms_median={k: round(float(np.median(v)), 4) for k, v in ms.items()},
                          ms_min={k: round(float(np.min(v)), 4) for k, v in ms.items()},
                          ms_max={k: round(float(np.max(v)), 4) for k, v in ms.items()})), flush=True)


if __name__ == "__main__":
    main()
