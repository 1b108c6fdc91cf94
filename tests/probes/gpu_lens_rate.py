"""Rates of the lens-camera render, on one GPU.  Nothing here is a test.

rt_render_lens_device (PERSPECTIVE at aperture 0 and with a lens; EQUIRECT) against rt_render_tiles_device on the FULL tile list --
the existing kernel with the same integrator and the same shape -- on the same build: HIP events on one stream, a warm-up round, then
interleaved rounds (tiles, pinhole, lens, panorama, tiles, ...), medians, and the yardstick's own spread (max - min over median).
1080p x 16 passes, MIS.  The two kernels differ in START only; the frames differ (other draws; a panorama sees other things), so a
ratio compares cost per frame, not the same paths.

usage: python tests/probes/gpu_lens_rate.py [--pairs N] [--small] > profiles/<name>.log"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import scenes  # noqa: E402

abi = scenes.abi
LENS_APERTURE = 0.1  # where the scene's own aperture is 0 (every scene file of tests/golden has 0)


def load(name):
    if name == "mesh1m":
        return scenes.random_triangle_mesh(1_000_000), scenes.MESH_CAMERA
    if name == "all_materials":
        return scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA
    ls = scenes.load_ssml(name)
    return ls.scene, ls.camera_params


def event_ms(torch, fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn(stream.cuda_stream)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="640 x 360 (a quick look; the numbers of section 23 are 1080p)")
    ap.add_argument("--scenes", default="rtweekend1,all_materials,mesh1m")
    args = ap.parse_args()
    import torch
    import bench
    hb = importlib.import_module("raytracing-rust_amd.hip_backend")
    w, h = (640, 360) if args.small else (1920, 1080)
    n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
    stream = torch.cuda.Stream()
    frame = torch.zeros(3 * w * h, dtype=torch.float32, device="cuda:0")
    d_tiles = torch.arange(n_tiles, dtype=torch.int32, device="cuda:0")
    for name in args.scenes.split(","):
        sc, cam_params = load(name)
        gpu, cam = hb.HipScene(sc, device=0), hb.camera_new(**cam_params)
        aperture = cam_params["aperture"] or LENS_APERTURE
        o = abi.default_render_opts(w, h, 16, method=abi.RT_METHOD_MIS, seed=1)
        o.sample_split = 0
        split = gpu.auto_sample_split(o)
        sums = torch.zeros(3 * max(split, 1) * 64 * n_tiles, dtype=torch.float32, device="cuda:0")
        d_sums = sums.data_ptr() if split > 1 else None

        def lens(projection, ap_):
            c = hb.lens_camera_new(**dict(cam_params, aperture=ap_), projection=projection)
            return lambda s: gpu.render_lens_device(c, o, frame.data_ptr(), d_sums, stream=s)
        runs = {"tiles": lambda s: gpu.render_tiles_device(cam, o, d_tiles.data_ptr(), n_tiles, frame.data_ptr(), d_sums, stream=s),
                "pinhole": lens("perspective", 0.0), "lens": lens("perspective", aperture), "equirect": lens("equirect", 0.0)}
        for fn in runs.values():  # warm-up
            event_ms(torch, fn, stream)
        ms = {k: [] for k in runs}
        for _ in range(args.pairs):
            for k, fn in runs.items():
                ms[k].append(event_ms(torch, fn, stream))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"scene": name, "size": [w, h], "passes": 16, "split": split, "aperture": aperture, "median_ms": med,
                          "ratio_to_tiles": {k: med[k] / med["tiles"] for k in runs if k != "tiles"},
                          "tiles_spread": (max(ms["tiles"]) - min(ms["tiles"])) / med["tiles"], "all_ms": ms,
                          "source_hash": bench.source_hash()}), flush=True)


if __name__ == "__main__":
    main()
