"""Cost of the bloom stage at 1920 x 1080, six levels.
  --mode events   (default) HIP events on one stream, REPS repetitions after a warm-up, the three calls interleaved:
                    bloom_fused   rt_bloom_device with fuse_tail 1
                    bloom_plain   rt_bloom_device with fuse_tail 0 (2n launches)
                    display       rt_display_device on the same frame, for scale
                  the frame is log-normal HDR noise (a tenth of it above the threshold); median, min and max per call, and the
                  run-to-run spread (max - min) next to the difference of the two bloom medians: the default is whichever is
                  faster by more than that spread.
  --mode kernels  REPS calls of both bloom variants: run it under
                  `rocprofv3 --kernel-trace --stats -- python tests/probes/gpu_bloom_rate.py --mode kernels` and read the kernels'
                  order and times.
  python tests/probes/gpu_bloom_rate.py [--mode M] [--reps N]
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

W, H, LEVELS = 1920, 1080, 6


def _arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


MODE = _arg("--mode", "events")
REPS = int(_arg("--reps", "31"))
WARM = 5


def _emit(**kw):
    print(json.dumps(dict(kw, size=f"{W}x{H}", levels=LEVELS, lib=os.path.basename(hb.LIB_PATH), reps=REPS,
                          source_hash=bench.source_hash())), flush=True)


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
    g = hb.HipScene(scenes.load_ssml("rtweekend1").scene, device=0)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    rng = np.random.default_rng(1)
    img = (rng.uniform(0.2, 1.0, (H, W, 3)) * np.exp2(rng.normal(-2.5, 2.0, (H, W, 1)))).astype(np.float32)
    rgb = torch.from_numpy(img).to(dev)
    out = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    opts = {fuse: hb.bloom_opts(W, H, levels=LEVELS, fuse_tail=fuse) for fuse in (0, 1)}
    ws = torch.zeros(hb.bloom_workspace_bytes(opts[1]), dtype=torch.uint8, device=dev)
    dopts = hb.display_opts(W, H)
    dws = torch.zeros(hb.display_workspace_bytes(dopts), dtype=torch.uint8, device=dev)
    px = torch.zeros(hb.display_output_bytes(dopts), dtype=torch.uint8, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    calls = {
        "bloom_fused": lambda: g.bloom_device(rgb.data_ptr(), opts[1], 0, ws.data_ptr(), out.data_ptr(), stream=s),
        "bloom_plain": lambda: g.bloom_device(rgb.data_ptr(), opts[0], 0, ws.data_ptr(), out.data_ptr(), stream=s),
        "display": lambda: g.display_device(rgb.data_ptr(), dopts, state.data_ptr(), dws.data_ptr(), px.data_ptr(), stream=s),
    }
    torch.cuda.synchronize()
    if MODE == "kernels":
        for _ in range(REPS):
            calls["bloom_fused"]()
            calls["bloom_plain"]()
            torch.cuda.synchronize()
        _emit(mode=MODE)
        return
    ms = {k: [] for k in calls}
    for rep in range(REPS + WARM):
        for k, fn in calls.items():
            t = _timed(stream, fn)
            if rep >= WARM:
                ms[k].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(np.max(v) - np.min(v)) for k, v in ms.items()}
    _emit(mode=MODE, above_threshold=round(float((img.max(axis=-1) > 1.0).mean()), 4),
          ms_median={k: round(v, 4) for k, v in med.items()}, ms_min={k: round(float(np.min(v)), 4) for k, v in ms.items()},
          ms_max={k: round(float(np.max(v)), 4) for k, v in ms.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
          fused_minus_plain_ms=round(med["bloom_fused"] - med["bloom_plain"], 4),
          frame_bytes_read_and_written=2 * 12 * n, gb_per_s_fused=round(2 * 12 * n / med["bloom_fused"] / 1e6, 1))


if __name__ == "__main__":
    main()
