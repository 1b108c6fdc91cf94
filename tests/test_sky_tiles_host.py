"""The two-sphere kernels' per-tile sky proof (csrc/rt_sky_tiles.h) on the CPU: tests/cpp/sky_tiles_check.cpp forms the launch
constants as a render does, classifies every 8 x 8 tile with the code the kernels inline, and runs the repository's own sphere_t on
every pixel of every flagged tile -- the four footprint corners, 32 points along each footprint edge and 64 seeded interior jitters,
directions through ray_new's normalisation.  Not one ray may hit either sphere; and each scene must be flagged the way its geometry
says.  tests/test_gpu_sky_run.py compares the same flags with the device's.

A tile is flagged only when its eight neighbours pass as well (the tile rule of the header), so a sphere smaller than a pixel clears
its own tile and all eight around it, wherever in its tile it lies."""
import numpy as np
import pytest

import sky_tiles_cases as cases

PER_PIXEL = 4 + 4 * 32 + 64


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_no_ray_of_a_flagged_tile_hits_a_sphere(hb, tmp_path_factory, name, size):
    width, height = size
    flags, counts = cases.host_run(hb, tmp_path_factory, name, width, height)
    tiles, flagged = counts["tiles"]
    pixels, rays, hits = counts["rays"]
    assert tiles == flags.size and flagged == int(flags.sum())
    assert rays == pixels * PER_PIXEL
    assert hits == 0, (name, size, hits)
    if name == "inside":
        assert flagged == 0
    if name == "behind":
        assert flagged == tiles and pixels == width * height
    if name == "rtweekend1" and size == (240, 135):
        assert 0.30 <= flagged / tiles <= 0.60, flagged / tiles  # a proof that never fires cannot pass
    if name in ("grazing", "tilted150") and size == (240, 135):
        assert flagged > 0  # the horizon and the wide view leave whole tiles of sky


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_subpixel_sphere_clears_its_tile_and_all_eight_neighbours(hb, tmp_path_factory, size):
    width, height = size
    flags, _ = cases.host_run(hb, tmp_path_factory, "subpixel", width, height)
    # the camera looks at the sphere: its direction is the image centre, u = v = 1/2, i.e. jittered coordinates ((W-1)/2, (H-1)/2)
    px, py = int(np.floor((width - 1) / 2.0)), int(np.floor((height - 1) / 2.0))
    tx, ty = px // 8, py // 8
    assert 0 < tx < flags.shape[1] - 1 and 0 < ty < flags.shape[0] - 1  # all eight neighbours exist
    assert not flags[ty - 1:ty + 2, tx - 1:tx + 2].any(), flags[ty - 1:ty + 2, tx - 1:tx + 2]
    # far from it everything is sky
    assert flags[0, 0] == 1 and flags[-1, -1] == 1
