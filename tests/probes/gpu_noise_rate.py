"""Cost of the noise estimates at 1920 x 1080.
  --mode kernels   REPS calls of rt_render_noise_device (all outputs) at SPP passes, sample_split 16, on rtweekend1: run it under
                   `rocprofv3 --kernel-trace --stats -- python tests/probes/gpu_noise_rate.py --mode kernels` and read
                   noise_chunk_kernel and noise_tile_kernel next to combine_chunks_kernel, the fold of the same chunks that every
                   render at that split already pays.
  --mode tiles     the tile stage alone (rt_noise_tiles_device: the summary's reset and the tile kernel) on planes in device
                   memory, HIP events, the median of REPS after a warm-up.  RT_HIP_LIB selects another build of the library: the
                   A/B build of the tile kernel that sums through LDS (-DRT_NOISE_TILE_LDS).
  --mode denoised  rt_render_denoised_split against rt_render_denoised, same scene, passes and sample_split, blocking calls timed
                   on the host, interleaved, the median of REPS after a warm-up, on rtweekend1 and a 1 M-triangle mesh.
  python tests/probes/gpu_noise_rate.py --mode M [--reps N] [--spp N] [--scenes rtweekend1,mesh1m]
Prints one JSON line per measurement."""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("raytracing-rust_amd")
hb = importlib.import_module("raytracing-rust_amd.hip_backend")
abi = pkg.abi
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import scenes  # noqa: E402

W, H, SPLIT = 1920, 1080, 16


def _arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


MODE = _arg("--mode", "tiles")
REPS = int(_arg("--reps", "9"))
SPP = int(_arg("--spp", "64"))


def _scene(name):
    if name == "rtweekend1":
        ls = scenes.load_ssml("rtweekend1")
        return ls.scene, ls.camera_params
    return scenes.random_triangle_mesh(1_000_000), scenes.MESH_CAMERA


def _emit(**kw):
    print(json.dumps(dict(kw, size=f"{W}x{H}", lib=os.path.basename(hb.LIB_PATH), reps=REPS, source_hash=bench.source_hash())), flush=True)


def main():
    dev = torch.device("cuda", 0)
    n, n_tiles = W * H, ((W + 7) // 8) * ((H + 7) // 8)
    if MODE == "tiles":
        sc, cam_params = _scene("rtweekend1")
        g = hb.HipScene(sc, device=0)
        rng = np.random.default_rng(0)
        lum = torch.from_numpy(rng.uniform(0.05, 2.0, n).astype(np.float32)).to(dev)
        var = torch.from_numpy((rng.uniform(0.0, 0.2, n) ** 2).astype(np.float32)).to(dev)
        err = torch.zeros(n_tiles, dtype=torch.float32, device=dev)
        summary = torch.zeros(4, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        ms = []
        for rep in range(REPS + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            g.noise_tiles_device(lum.data_ptr(), var.data_ptr(), W, H, err.data_ptr(), summary.data_ptr(), stream=stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            if rep >= 3:
                ms.append(a.elapsed_time(b))
        s = summary.cpu().numpy()
        _emit(mode=MODE, tile_stage_ms_median=round(float(np.median(ms)), 4), tile_stage_ms_min=round(float(np.min(ms)), 4),
              tiles=n_tiles, tiles_above=int(s[1]), max_tile_error=float(s[:1].view(np.float32)[0]))
        return
    for name in _arg("--scenes", "rtweekend1" if MODE == "kernels" else "rtweekend1,mesh1m").split(","):
        sc, cam_params = _scene(name)
        g = hb.HipScene(sc, device=0)
        cam = hb.camera_new(**cam_params)
        opts = abi.default_render_opts(W, H, SPP, seed=1)
        opts.sample_split = SPLIT
        if MODE == "kernels":
            out = {"mean": torch.zeros(3 * n, dtype=torch.float32, device=dev), "variance": torch.zeros(n, dtype=torch.float32, device=dev),
                   "lum_mean": torch.zeros(n, dtype=torch.float32, device=dev), "tile_error": torch.zeros(n_tiles, dtype=torch.float32, device=dev),
                   "summary": torch.zeros(4, dtype=torch.int32, device=dev)}
            for _ in range(REPS):
                g.render_noise_device(cam, opts, {k: t.data_ptr() for k, t in out.items()})
                torch.cuda.synchronize()
            _emit(mode=MODE, scene=name, spp=SPP, split=SPLIT, render_ms=round(g.last_kernel_ms()[0], 3))
        else:
            fns = [lambda: g.render_denoised(cam, opts), lambda: g.render_denoised_split(cam, opts)]
            secs = [[], []]
            for rep in range(REPS + 1):
                for i, fn in enumerate(fns):
                    t0 = time.perf_counter()
                    fn()
                    if rep >= 1:
                        secs[i].append(time.perf_counter() - t0)
            two, one = (float(np.median(s)) * 1e3 for s in secs)
            _emit(mode=MODE, scene=name, spp=SPP, split=SPLIT, render_denoised_ms=round(two, 2), render_denoised_split_ms=round(one, 2),
                  split_over_halves=round(one / two, 4))


if __name__ == "__main__":
    main()
