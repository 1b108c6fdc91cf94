"""Rates of the tile-list render and the adaptive loop, on one GPU.  Nothing here is a test.

  (a) rt_render_tiles_device on the FULL tile list against rt_render_device at the same opts: HIP events on one stream, a warm-up,
      then interleaved pairs (A B A B ...), medians.  1080p x 16 passes, MIS, the scenes of section 21's table.
  (b) rt_render_adaptive against rt_render_converged at the same batch, threshold and max_passes (wall time of the blocking
      calls, interleaved, medians), pixel_passes over W * H * passes, and the crossover: rt_render_tiles_device on the first
      fraction f of the tile list against the whole-frame launch, for f = 1/64 ... 1.
  (c) is bench.py itself, run on this commit and on its parent on the same machine.

usage: python tests/probes/gpu_adaptive_rate.py [--pairs N] [--small] > profiles/<name>.log"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import scenes  # noqa: E402

abi = scenes.abi


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
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="640 x 360 (a quick look; the numbers of section 22 are 1080p)")
    ap.add_argument("--scenes", default="rtweekend1,overshadowed,all_materials,mesh1m")
    args = ap.parse_args()
    import torch
    hb = importlib.import_module("raytracing-rust_amd.hip_backend")
    w, h = (640, 360) if args.small else (1920, 1080)
    n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
    stream = torch.cuda.Stream()
    frame = torch.zeros(3 * w * h, dtype=torch.float32, device="cuda:0")
    d_tiles = torch.arange(n_tiles, dtype=torch.int32, device="cuda:0")
    for name in args.scenes.split(","):
        sc, cam_params = load(name)
        gpu, cam = hb.HipScene(sc, device=0), hb.camera_new(**cam_params)
        o = abi.default_render_opts(w, h, 16, method=abi.RT_METHOD_MIS, seed=1)
        o.sample_split = 0
        split = gpu.auto_sample_split(o)
        sums = torch.zeros(3 * max(split, 1) * 64 * n_tiles, dtype=torch.float32, device="cuda:0")
        render = lambda s: gpu.render_device(cam, o, frame.data_ptr(), stream=s)

        def tiles(n, with_sums=True):
            return lambda s: gpu.render_tiles_device(cam, o, d_tiles.data_ptr(), n, frame.data_ptr(), sums.data_ptr() if with_sums and split > 1 else None, stream=s)
        for fn in (render, tiles(n_tiles)):  # warm-up (and the scene's scratch grows here)
            event_ms(torch, fn, stream)
        ta, tb = [], []
        for _ in range(args.pairs):
            ta.append(event_ms(torch, render, stream))
            tb.append(event_ms(torch, tiles(n_tiles), stream))
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(json.dumps({"part": "a", "scene": name, "size": [w, h], "passes": 16, "split": split, "render_ms": ma, "tiles_ms": mb,
                          "ratio": mb / ma, "render_all": ta, "tiles_all": tb}), flush=True)
        if name not in ("rtweekend1", "all_materials"):
            continue
        cross = []
        for k in (64, 32, 16, 8, 4, 2, 1):
            n = max(1, n_tiles // k)
            event_ms(torch, tiles(n), stream)
            ts = [event_ms(torch, tiles(n), stream) for _ in range(args.pairs)]
            cross.append({"fraction": n / n_tiles, "tiles_ms": statistics.median(ts), "vs_whole_frame": statistics.median(ts) / ma})
        print(json.dumps({"part": "b-crossover", "scene": name, "whole_frame_ms": ma, "masked": cross}), flush=True)
        ob = abi.default_render_opts(w, h, 16, method=abi.RT_METHOD_MIS, seed=1)
        ob.sample_split = 4  # (the automatic split of 16 passes at 1080p is 1: no estimate)
        kw = dict(min_batches=2, max_passes=8 * 16)
        gpu.render_adaptive(cam, ob, 16, **kw)
        gpu.render_converged(cam, ob, 16, **kw)
        wa, wc = [], []
        for _ in range(3):
            t = time.perf_counter()
            ra = gpu.render_adaptive(cam, ob, 16, **kw)
            wa.append(time.perf_counter() - t)
            t = time.perf_counter()
            rc = gpu.render_converged(cam, ob, 16, **kw)
            wc.append(time.perf_counter() - t)
        whole_s = (ma / 1e3) * min(ra["batches"], 2)
        print(json.dumps({"part": "b", "scene": name, "adaptive_s": statistics.median(wa), "converged_s": statistics.median(wc),
                          "adaptive_batches": ra["batches"], "converged_batches": rc["batches"], "adaptive_converged": ra["converged"],
                          "work_fraction": ra["pixel_passes"] / (w * h * ra["batches"] * 16),
                          "masked_share_of_time_estimate": max(0.0, 1.0 - whole_s / statistics.median(wa))}), flush=True)


if __name__ == "__main__":
    main()
