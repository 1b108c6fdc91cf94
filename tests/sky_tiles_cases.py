"""The scenes, cameras and frame sizes the per-tile sky proof (csrc/rt_sky_tiles.h) is tested on, shared by the host check
(tests/test_sky_tiles_host.py) and the GPU tests (tests/test_gpu_sky_run.py), and the one way both run tests/cpp/sky_tiles_check.cpp.
A plain module: the tests import it."""
import numpy as np

import host_check
import scenes

abi = scenes.abi

SIZES = ((64, 40), (97, 53), (240, 135))  # 97 x 53: edge tiles on both axes

RTWEEKEND1 = (((0.0, 1.0, -100.5), 100.0), ((0.0, 1.0, 0.0), 0.5))  # tests/golden/scenes/rtweekend1.ssml
_FORWARD = dict(origin=(0.0, 0.0, 0.0), lookat=(0.0, 1.0, 0.0), vup=(0.0, 0.0, 1.0), fov=60.0, aperture=0.0, focus_dist=1.0)


def _rtweekend1_camera():
    p = dict(scenes.load_ssml("rtweekend1").camera_params)
    p.pop("aspect_ratio", None)
    return p


# name -> (spheres ((centre, radius), (centre, radius)), camera parameters without the aspect ratio: the frame's own is used)
CASES = {
    "rtweekend1": (RTWEEKEND1, _rtweekend1_camera()),
    # the origin inside the large sphere: nothing may be flagged
    "inside": (RTWEEKEND1, dict(_FORWARD, origin=(0.0, 1.0, -50.0), lookat=(0.0, 2.0, -50.0))),
    # both spheres behind the camera: every tile is flagged (the lines of sight meet them behind the origin)
    "behind": ((((0.0, -5.0, 0.0), 1.0), ((0.5, -9.0, 0.3), 2.0)), _FORWARD),
    # a sphere smaller than a pixel at the image centre (the other one behind the camera)
    "subpixel": ((((0.0, 10.0, 0.0), 0.01), ((0.0, -5.0, 0.0), 1.0)), _FORWARD),
    # radius 1e4 at distance 1.0001e4: a grazing horizon
    "grazing": ((((0.0, 0.0, -1.0001e4), 1.0e4), ((0.0, 5.0, 1.0), 0.5)), _FORWARD),
    # vup not axis-aligned, a narrow and a very wide field of view
    "tilted20": (RTWEEKEND1, dict(_FORWARD, vup=(0.3, 0.2, 0.9), fov=20.0, lookat=(0.2, 1.0, 0.8))),
    "tilted150": (RTWEEKEND1, dict(_FORWARD, vup=(0.3, 0.2, 0.9), fov=150.0, lookat=(0.2, 1.0, -0.1))),
}


def camera_params(name, width, height):
    return dict(CASES[name][1], aspect_ratio=float(np.float32(width) / np.float32(height)))


def scene(name):
    """the case as a scene the two-sphere kernels take: two Lambertian spheres under a lerp sky with a sampled table"""
    sc = scenes.SceneDescription()
    grey = sc.lambertian(sc.solid((0.5, 0.5, 0.5)), 1.0)
    for centre, radius in CASES[name][0]:
        sc.sphere(centre, radius, grey)
    sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (16, 8))
    return sc


_PROGRAM = {}


def program(tmp_path_factory):
    """tests/cpp/sky_tiles_check.cpp, built once per session with AddressSanitizer and UBSan"""
    if "exe" not in _PROGRAM:
        _PROGRAM["exe"] = host_check.build("sky_tiles_check", tmp_path_factory.mktemp("sky_tiles_check"), sanitize=True)
    return _PROGRAM["exe"]


_RESULTS = {}


def host_run(hb, tmp_path_factory, name, width, height):
    """(flags (tiles_y, tiles_x) uint8, the program's counts {"tiles", "rays", "block"}) of the case at that size, run once per session"""
    key = (name, width, height)
    if key not in _RESULTS:
        cam = hb.camera_new(**camera_params(name, width, height))
        spheres = CASES[name][0]
        floats = [*spheres[0][0], spheres[0][1], *spheres[1][0], spheres[1][1], *cam.origin, *cam.lower_left, *cam.horizontal, *cam.vertical]
        words = [int(np.float32(v).view(np.uint32)) for v in floats]
        out = str(tmp_path_factory.mktemp("sky_flags") / "flags.bin")
        counts = host_check.run(program(tmp_path_factory), out, width, height, *words, timeout=300)
        flags = np.fromfile(out, dtype=np.uint8).reshape((height + 7) // 8, (width + 7) // 8)
        _RESULTS[key] = (flags, counts)
    return _RESULTS[key]
