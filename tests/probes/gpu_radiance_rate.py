"""Rate of the radiance queries at 1920 x 1080: rt_radiance_device on the pixel-centre rays of the scene's
camera at K samples a ray, MIS, against rt_render_device of the same scene, size, method and K passes on the same build -- same
box, interleaved, REPS pairs after a warm-up pair, HIP events around each call.  Not a test: run it by hand,
  timeout -k 10 600 python tests/probes/gpu_radiance_rate.py [--reps 5] [--samples 16] [--scenes rtweekend1,overshadowed,all_materials,mesh1m]
one process per invocation; a caller that measures several builds (RT_HIP_LIB: e.g. -DRT_RADIANCE_QUORUM=16 / 48 through the
Makefile's EXTRA) runs it once per build, each under its own time limit.  Prints one JSON line per scene."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
pkg = importlib.import_module("raytracing-rust_amd")
hb = importlib.import_module("raytracing-rust_amd.hip_backend")
abi = pkg.abi
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import radiance_checker as R  # noqa: E402
import scenes  # noqa: E402

W, H = 1920, 1080


def _arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


REPS = int(_arg("--reps", "5"))
SAMPLES = int(_arg("--samples", "16"))


def _scene(name):
    if name in ("rtweekend1", "overshadowed"):
        ls = scenes.load_ssml(name)
        return ls.scene, ls.camera_params
    if name == "all_materials":
        return scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA
    return scenes.random_triangle_mesh(1_000_000), scenes.MESH_CAMERA


def main():
    dev = torch.device("cuda", 0)
    n = W * H
    for name in _arg("--scenes", "rtweekend1,overshadowed,all_materials,mesh1m").split(","):
        sc, cam_params = _scene(name)
        g = hb.HipScene(sc, device=0)
        cam = hb.camera_new(**cam_params)
        o, d = R.pixel_centre_rays(cam, W, H)
        rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([o, d], axis=1))).to(dev)
        out_q = torch.zeros(3 * n, dtype=torch.float32, device=dev)
        out_r = torch.zeros(3 * n, dtype=torch.float32, device=dev)
        opts = abi.default_render_opts(W, H, SAMPLES, method=abi.RT_METHOD_MIS, seed=1)
        stream = torch.cuda.Stream(device=dev)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        query = lambda: g.radiance_device(rays.data_ptr(), 0, n, out_q.data_ptr(), method=abi.RT_METHOD_MIS, samples=SAMPLES, seed=1,  # noqa: E731
                                          stream=stream.cuda_stream)
        render = lambda: g.render_device(cam, opts, out_r.data_ptr(), stream=stream.cuda_stream)  # noqa: E731
        ms = [[], []]
        for rep in range(REPS + 1):  # (the first pair warms up)
            for i, fn in enumerate((query, render)):
                t = timed(fn)
                if rep >= 1:
                    ms[i].append(t)
        q, r = float(np.median(ms[0])), float(np.median(ms[1]))
        total = n * SAMPLES
        print(json.dumps(dict(scene=name, size=f"{W}x{H}", samples=SAMPLES, method="mis", reps=REPS, radiance_ms=[round(x, 3) for x in ms[0]],
                              render_ms=[round(x, 3) for x in ms[1]], radiance_msamples_per_s=round(total / q / 1e3, 2),
                              render_msamples_per_s=round(total / r / 1e3, 2), radiance_over_render_time=round(q / r, 3),
                              render_kernel=g.last_launch_info()["kernel"], lib=os.path.basename(hb.LIB_PATH),
                              source_hash=bench.source_hash())), flush=True)


if __name__ == "__main__":
    main()
