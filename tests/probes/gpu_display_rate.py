"""Cost of the display stage (rt_display_device) per call, timed with HIP events on one stream after a warm-up, at 1920 x 1080 and
3840 x 2160 (a rendered rtweekend1 frame, 1 pass, tiled up to the size).  Rows:
  auto_aces_srgb_dither_rgba8    the full AUTO path with a state
  fixed_reference_rgb8           FIXED + CLAMP + GAMMA 2.2 + REFERENCE + RGB8 ...
  output_rgb8_device             ... next to the reference conversion it reproduces
  constant_image_auto            every pixel in one histogram bin: the worst case for the LDS atomics
  python tests/probes/gpu_display_rate.py [--reps N]
Prints one JSON line: ms (median of N, default 9).  Per-kernel times: run this under rocprofv3 --kernel-trace --stats in a run of
its own."""
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

import scenes  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9


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
    ls = scenes.load_ssml("rtweekend1")
    gpu = hb.HipScene(ls.scene, device=0)
    cam = hb.camera_new(**ls.camera_params)
    base, _ = gpu.render(cam, abi.default_render_opts(1920, 1080, 1, method=abi.RT_METHOD_MIS, seed=1))
    stream = torch.cuda.Stream(device=dev)
    h_stream = stream.cuda_stream
    result = {"probe": "gpu_display_rate", "reps": REPS, "ms": {}}
    for w, h in ((1920, 1080), (3840, 2160)):
        img = np.tile(base, (h // 1080, w // 1920, 1))
        src = torch.from_numpy(np.ascontiguousarray(img)).to(dev).reshape(-1)
        flat = torch.full_like(src, 0.3)
        state = torch.zeros(4, dtype=torch.int32, device=dev)
        hist = torch.zeros(256, dtype=torch.int32, device=dev)
        out = torch.zeros(w * h * 4, dtype=torch.uint8, device=dev)
        rows = {}
        for row, data, kw in (("auto_aces_srgb_dither_rgba8", src, dict(adaptation=0.3)),
                              ("fixed_reference_rgb8", src, dict(exposure_mode="fixed", tonemap="clamp", transfer="gamma",
                                                                 quantiser="reference", pixel_format="rgb8")),
                              ("constant_image_auto", flat, dict(adaptation=0.3))):
            o = hb.display_opts(w, h, **kw)
            ws = torch.empty(hb.display_workspace_bytes(o), dtype=torch.uint8, device=dev)
            rows[row] = timed(stream, lambda: gpu.display_device(data.data_ptr(), o, state.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                                                 hist.data_ptr(), stream=h_stream))
        rows["output_rgb8_device"] = timed(stream, lambda: gpu.output_rgb8_device(src.data_ptr(), w * h * 3, out.data_ptr(), 2.2,
                                                                                  h_stream))
        result["ms"][f"{w}x{h}"] = rows
    print(json.dumps(result))


if __name__ == "__main__":
    main()
