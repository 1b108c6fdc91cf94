"""Cost of the ID-matte stage: the layer kernel (rt_render_matte_device, K = 4 and 8, both ID kinds) next to the first-hit AOV
pass with only its two ID channels (rt_render_aov_device) over the same window -- the same walks, so the yardstick --, and the
extraction kernel (rt_matte_extract_device) next to its compulsory bytes, (8 K + 4) per pixel.  HIP events on one stream, the
median of N after a warm-up, the layer and AOV passes interleaved in one process: rtweekend1.ssml and a 1 M-triangle random mesh,
1920 x 1080 x 16.
  python tests/probes/gpu_matte_rate.py [--reps N]
Prints one JSON line per scene, ID kind and K."""
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
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7


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
    ls = scenes.load_ssml("rtweekend1")
    cases = [("rtweekend1", ls.scene, ls.camera_params), ("mesh1m", scenes.random_triangle_mesh(1_000_000), scenes.MESH_CAMERA)]
    n = W * H
    ids = torch.zeros(8 * n, dtype=torch.int32, device=dev)
    cov = torch.zeros(8 * n, dtype=torch.float32, device=dev)
    res = torch.zeros(n, dtype=torch.float32, device=dev)
    out = torch.zeros(n, dtype=torch.float32, device=dev)
    aov = {name: torch.zeros(n, dtype=torch.int32, device=dev) for name in ("primitive", "material")}
    aov_ptrs = {name: t.data_ptr() for name, t in aov.items()}
    matte_ptrs = {"ids": ids.data_ptr(), "coverage": cov.data_ptr(), "residual": res.data_ptr()}
    for name, sc, cam_params in cases:
        g = hb.HipScene(sc, device=0)
        cam = hb.camera_new(**cam_params)
        opts = abi.default_render_opts(W, H, SPP, seed=1)
        for kind in ("material", "primitive"):
            for k in (4, 8):
                with torch.cuda.stream(stream):
                    aov_ms, matte_ms = timed_interleaved(stream, [
                        lambda: g.render_aov_device(cam, opts, aov_ptrs, stream=stream.cuda_stream),
                        lambda: g.render_matte_device(cam, opts, matte_ptrs, id_kind=kind, layers=k, stream=stream.cuda_stream)])
                    # the IDs the layers hold, every other one selected (ascending, as the device call wants them)
                    stream.synchronize()
                    occupied = cov[:k * n].cpu().numpy() > 0
                    present = np.unique(ids[:k * n].cpu().numpy().view(np.uint32)[occupied])
                    sel = torch.from_numpy(present[::2].view(np.int32).copy()).to(dev)
                    extract_ms, = timed_interleaved(stream, [
                        lambda: g.matte_extract_device(ids.data_ptr(), cov.data_ptr(), W, H, k, sel.data_ptr(), sel.numel(),
                                                       out.data_ptr(), stream=stream.cuda_stream)])
                    layers_used = float(occupied.sum()) / n
                extract_bytes = (8 * k + 4) * n
                print(json.dumps({"scene": name, "size": f"{W}x{H}x{SPP}", "id_kind": kind, "layers": k,
                                  "aov_ids_ms": round(aov_ms, 3), "matte_ms": round(matte_ms, 3),
                                  "matte_over_aov": round(matte_ms / aov_ms, 3),
                                  "matte_primary_rays_per_s": round(n * SPP / (matte_ms * 1e-3)),
                                  "mean_occupied_layers": round(layers_used, 3), "selected_ids": int(sel.numel()),
                                  "extract_ms": round(extract_ms, 4), "extract_compulsory_bytes": extract_bytes,
                                  "extract_gb_per_s": round(extract_bytes / (extract_ms * 1e-3) / 1e9, 1),
                                  "reps": REPS, "source_hash": bench.source_hash()}), flush=True)


if __name__ == "__main__":
    main()
