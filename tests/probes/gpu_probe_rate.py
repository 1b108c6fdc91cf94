"""Rates of the light probes, on one GPU.  Nothing here is a test.

rt_probe_sh_device (4096 probes on a 16 x 16 x 16 grid through the scene's box, K = 1024, S = 64, MIS) against the unchanged
rt_radiance_device on the SAME NUMBER of rays from the same positions -- one rt_ray_desc per sample, uniformly distributed directions
uploaded beforehand, K = 1 -- on the same build: HIP events on one stream, a warm-up round, then interleaved rounds (radiance, probe,
radiance, ...), medians, and the yardstick's own spread (max - min over median).  The two kernels share the integrator; the probe
kernel adds the two direction draws, rt_sinf / rt_cosf and the 27 read-add-writes of its record per sample, and a (probe, chunk)
hand-out in place of one lane per ray.  The directions differ (other draws), so a ratio compares cost per sample, not the same paths.

usage: python tests/probes/gpu_probe_rate.py [--pairs N] [--small] > profiles/<name>.log"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import scenes  # noqa: E402

abi = scenes.abi


def load(name):
    if name == "mesh1m":
        return scenes.random_triangle_mesh(1_000_000)
    if name == "all_materials":
        return scenes.all_materials()
    return scenes.load_ssml(name).scene


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
    ap.add_argument("--small", action="store_true", help="512 probes x 64 samples, S = 8 (a quick look; the numbers of section 25 are 4096 x 1024)")
    ap.add_argument("--scenes", default="rtweekend1,all_materials,mesh1m")
    args = ap.parse_args()
    import torch
    import bench
    hb = importlib.import_module("raytracing-rust_amd.hip_backend")
    side, k, split = (8, 64, 8) if args.small else (16, 1024, 64)
    n = side ** 3
    o = dict(render_method=abi.RT_METHOD_MIS, samples_per_probe=k, sample_split=split, seed=1)
    stream = torch.cuda.Stream()
    for name in args.scenes.split(","):
        gpu = hb.HipScene(load(name), device=0)
        root = gpu.nodes()[0]
        lo, hi = np.array(root["min"], np.float64), np.array(root["max"], np.float64)
        t = (np.arange(side) + 0.5) / side
        grid = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)
        pos = (lo + grid * (hi - lo)).astype(np.float32)
        d_pos = torch.from_numpy(pos).to("cuda:0")
        d_out = torch.zeros(27 * n, dtype=torch.float32, device="cuda:0")
        d_work = torch.zeros(hb.probe_workspace_bytes(n, **o) // 4, dtype=torch.float32, device="cuda:0")
        # the yardstick's rays: every position k times, directions uniform on the sphere (normalised Gaussians), made on the device
        g = torch.Generator(device="cuda:0").manual_seed(1)
        dirs = torch.randn((n * k, 3), generator=g, device="cuda:0", dtype=torch.float32)
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        d_rays = torch.cat([d_pos.repeat_interleave(k, dim=0), dirs], dim=1).contiguous()
        del dirs
        d_rgb = torch.zeros(3 * n * k, dtype=torch.float32, device="cuda:0")
        runs = {"radiance": lambda s: gpu.radiance_device(d_rays.data_ptr(), 0, n * k, d_rgb.data_ptr(), method=abi.RT_METHOD_MIS, samples=1, seed=1, stream=s),
                "probe": lambda s: gpu.probe_sh_device(d_pos.data_ptr(), n, d_out.data_ptr(), d_work.data_ptr(), None, stream=s, **o)}
        for fn in runs.values():  # warm-up
            event_ms(torch, fn, stream)
        ms = {key: [] for key in runs}
        for _ in range(args.pairs):
            for key, fn in runs.items():
                ms[key].append(event_ms(torch, fn, stream))
        med = {key: statistics.median(v) for key, v in ms.items()}
        print(json.dumps({"scene": name, "probes": n, "samples_per_probe": k, "sample_split": split, "rays": n * k, "median_ms": med,
                          "ratio_probe_to_radiance": med["probe"] / med["radiance"],
                          "radiance_spread": (max(ms["radiance"]) - min(ms["radiance"])) / med["radiance"], "all_ms": ms,
                          "source_hash": bench.source_hash()}), flush=True)
        del d_rays, d_rgb, d_work


if __name__ == "__main__":
    main()
