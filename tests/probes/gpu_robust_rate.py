"""Cost of the firefly-robust combine at 1920 x 1080, sample_split 16 and 64.
  --mode events   (default) for each split, HIP events on one stream, REPS repetitions after a warm-up, the calls interleaved:
                    render    rt_render_device at that split: the render kernel and combine_chunks_kernel
                    noise     rt_render_noise_device (mean, variance): the same and noise_chunk_kernel
                    robust    rt_render_robust_device (mean given, every plane): the same and robust_chunk_kernel
                  all three on the same partial buffer, one pass per chunk (the render is as short as it gets).  The kernels'
                  own times are differences of medians: combine = render - rt_last_kernel_ms, noise_chunk = noise - render,
                  robust_chunk = robust - render.  Then robust_chunk_kernel ALONE, no difference taken: rt_robust_combine_device
                  on a caller's buffer of the same size (frame raster), per mode, with the bytes it must move -- the chunk sums
                  once for every pixel and a second time for the pixels that trim or drop something, plus what it writes --
                  over its time.
  --mode kernels  REPS calls of rt_render_noise_device and rt_render_robust_device at one split: run it under
                  `rocprofv3 --kernel-trace --stats -- python tests/probes/gpu_robust_rate.py --mode kernels --split 16` and read
                  robust_chunk_kernel next to noise_chunk_kernel and combine_chunks_kernel.
  python tests/probes/gpu_robust_rate.py [--mode M] [--reps N] [--split S]
Prints one JSON line per measurement."""
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


def _arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


MODE = _arg("--mode", "events")
REPS = int(_arg("--reps", "9"))
SPLITS = [int(_arg("--split", "0"))] if "--split" in sys.argv else [16, 64]
WARM = 3


def _emit(**kw):
    print(json.dumps(dict(kw, size=f"{W}x{H}", lib=os.path.basename(hb.LIB_PATH), reps=REPS, source_hash=bench.source_hash())), flush=True)


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
    f32 = lambda count: torch.zeros(count, dtype=torch.float32, device=dev)  # noqa: E731
    u8 = lambda count: torch.zeros(count, dtype=torch.uint8, device=dev)  # noqa: E731
    mean, out, gini, var, trimmed, dropped = f32(3 * n), f32(3 * n), f32(n), f32(n), u8(n), u8(n)
    robust_ptrs = {"out": out.data_ptr(), "mean": mean.data_ptr(), "gini": gini.data_ptr(), "trimmed": trimmed.data_ptr(),
                   "dropped": dropped.data_ptr()}
    for split in SPLITS:
        opts = abi.default_render_opts(W, H, split, seed=1)  # one pass per chunk
        opts.sample_split = split
        s = stream.cuda_stream
        calls = {
            "render": lambda: g.render_device(cam, opts, mean.data_ptr(), stream=s),
            "noise": lambda: g.render_noise_device(cam, opts, {"mean": mean.data_ptr(), "variance": var.data_ptr()}, stream=s),
            "robust": lambda: g.render_robust_device(cam, opts, robust_ptrs, stream=s, mode="median"),
        }
        if MODE == "kernels":
            for _ in range(REPS):
                calls["noise"]()
                calls["robust"]()
                torch.cuda.synchronize()
            _emit(mode=MODE, split=split, passes=split)
            continue
        ms = {k: [] for k in calls}
        kernel_ms = []
        for rep in range(REPS + WARM):
            for k, fn in calls.items():
                t = _timed(stream, fn)
                if rep >= WARM:
                    ms[k].append(t)
                    if k == "render":
                        kernel_ms.append(g.last_kernel_ms()[0])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        _emit(mode=MODE, what="differences of medians", split=split, passes=split, render_call_ms=round(med["render"], 4),
              render_kernel_ms=round(float(np.median(kernel_ms)), 4), noise_call_ms=round(med["noise"], 4), robust_call_ms=round(med["robust"], 4),
              combine_chunks_ms=round(med["render"] - float(np.median(kernel_ms)), 4), noise_chunk_ms=round(med["noise"] - med["render"], 4),
              robust_chunk_median_mode_ms=round(med["robust"] - med["render"], 4),
              spread_ms={k: round(float(np.max(v) - np.min(v)), 4) for k, v in ms.items()})
        # the kernel alone on a caller's buffer of the same size: uniform sums, one firefly chunk in every 16th pixel
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        sums = torch.rand((split, n, 3), generator=gen, dtype=torch.float32, device=dev)
        sums[split // 2, ::16] *= 1000.0
        for mode in ("median", "gini", "trim"):
            kw = dict(mode=mode, trim=0) if mode == "trim" else dict(mode=mode)
            t = [_timed(stream, lambda: g.robust_combine_device(sums.data_ptr(), split, 1, W, H, robust_ptrs, stream=s, **kw))
                 for _ in range(REPS + WARM)][WARM:]
            twice = float(((trimmed > 0) | (dropped > 0)).float().mean().item())
            moved = 12 * n * split * (1.0 + twice) + n * (12 + 12 + 4 + 1 + 1)
            med_ms = float(np.median(t))
            _emit(mode=MODE, what="rt_robust_combine_device alone", split=split, robust_mode=mode if mode != "trim" else "trim 0",
                  ms_median=round(med_ms, 4), ms_min=round(float(np.min(t)), 4), ms_max=round(float(np.max(t)), 4),
                  pixels_read_twice=round(twice, 4), bytes_moved=int(moved), gb_per_s=round(moved / med_ms / 1e6, 1),
                  floor_bytes_two_reads=2 * 12 * n * split)
        del sums


if __name__ == "__main__":
    main()
