"""The stream seed of GEN in the coarse two-sphere kernels (csrc/rt_gen_keys.h; the switches lean_gen_keys and
lean_gen_item_product of csrc/rt_lean.h): the Philox round keys from a table the host forms once per render, and the first round's
pixel product formed where a lane is handed its item.
(a) rt_selftest_gen_keys: the keyed seeding, without and with the product formed ahead, next to rt_rng_seed ON the device -- the
four state words and the first eight draws, bit for bit -- over seeds x pixels x sample indices x sample windows (the table below)
and seeded random cases, a launch per seed; one case is the counter whose Philox block is all zero, so the guard that keeps xoshiro
off the zero state runs on the device too.
(b) frames and ray counts of rtweekend1 at 72 x 40 (9 x 5 whole tiles of the default 8 x 8) and at 70 x 37 (the same 45 tiles, the
last column and the last row padded: lanes handed padding ask again), 8 passes, bit for bit against the oracle as
tests/test_gpu_parity.py compares frames, with the chunk hand-out and with whole-pixel items (whose later chunks start in finalize),
and against the general spheres-only kernel, which seeds through rt_rng_seed.
tests/test_gen_keys_host.py runs the same forms on the CPU."""
import numpy as np
import pytest

import scenes
from gpu_support import abi, assert_same_bits
from test_gen_keys_host import SEEDS
from test_gpu_parity import assert_images_match  # the parity tests' own comparison and tolerance

pytestmark = pytest.mark.gpu

PIXELS = (0, 1, 1 << 31, (1 << 32) - 1)
SAMPLE_INDICES = (0, 1)
# sample windows: sample_begin + sample index crosses 2^32 (the 64-bit stream case) and 2^64 (wraps) for index 1
SAMPLE_BEGINS = (0, 5, 0xFFFFFFFE, 0xFFFFFFFF, 0x100000000, 1 << 63, 0xDEADBEEFFFFFFFFF, 0xFFFFFFFFFFFFFFFF)
# the one counter with a pixel index below 2^32 whose Philox block is all zero under this seed (tests/cpp/gen_keys_check.cpp)
ZERO_SEED, ZERO_PIXEL, ZERO_SAMPLE = 0x806AB30FD9C60ABE, 0x1CCED5BF, 0xA2047F57D52EC01B
N_RANDOM = 4096


def cases_for(seed):
    """(n, 4) uint32: pixel, sample index, sample_begin low / high"""
    rows = [(p, i, b & 0xFFFFFFFF, b >> 32) for p in PIXELS for i in SAMPLE_INDICES for b in SAMPLE_BEGINS]
    rng = np.random.default_rng(seed & 0xFFFFFFFF)
    rnd = rng.integers(0, 1 << 32, (N_RANDOM, 4), dtype=np.uint64)
    rnd[:, 1] &= 0xFFFF  # a sample index is below spp
    rows = np.concatenate([np.array(rows, dtype=np.uint64), rnd]).astype(np.uint32)
    if seed == ZERO_SEED:  # the all-zero block: as index 0 of its window, and as index 1 of the window one below
        extra = [(ZERO_PIXEL, 0, ZERO_SAMPLE & 0xFFFFFFFF, ZERO_SAMPLE >> 32), (ZERO_PIXEL, 1, (ZERO_SAMPLE - 1) & 0xFFFFFFFF, (ZERO_SAMPLE - 1) >> 32)]
        rows = np.concatenate([rows, np.array(extra, dtype=np.uint32)])
    return rows


@pytest.mark.parametrize("seed", SEEDS, ids=[hex(s) for s in SEEDS])
def test_the_keyed_seed_is_rt_rng_seed_on_the_device(hb, seed):
    cases = cases_for(seed)
    res = hb.selftest_gen_keys(seed, cases)
    print(hex(seed), res)
    assert res["tested"] == len(cases) >= len(PIXELS) * len(SAMPLE_INDICES) * len(SAMPLE_BEGINS) + N_RANDOM, res
    assert res["state_mismatches"] == 0 and res["draw_mismatches"] == 0, res
    assert res["item_state_mismatches"] == 0 and res["item_draw_mismatches"] == 0, res
    assert res["zero_blocks"] == (2 if seed == ZERO_SEED else 0), res  # the guard ran exactly where the block is all zero
    assert set(res["in_use"]) <= set(abi.GEN_KEYS_FORM_NAMES), res
    assert "item_product" not in res["in_use"] or "key_table" in res["in_use"], res  # the product is carried only into the keyed form


def test_the_self_test_checks_its_arguments(hb):
    with pytest.raises(hb.RtHipError):
        hb.selftest_gen_keys(1, cases_for(1), device=99)
    with pytest.raises(ValueError):
        hb.selftest_gen_keys(1, np.zeros((4, 3), dtype=np.uint32))


FRAME_SEEDS = (1, 0xFFFFFFFF00000001)
FRAMES = ((72, 40), (70, 37))
METHODS = (abi.RT_METHOD_MIS, abi.RT_METHOD_NAIVE)


@pytest.fixture(scope="module")
def loaded(hb, O):
    ls = scenes.load_ssml("rtweekend1")
    general = hb.HipScene(ls.scene, device=0)
    general.set_tuning(abi.RT_TUNE_FEATURE_SET, 0)
    return hb.HipScene(ls.scene, device=0), general, O.Scene(ls.scene), ls.camera_params


@pytest.fixture(scope="module")
def references(O, loaded):
    """the oracle's frame and ray count per (frame, seed, split, method), rendered once (the share is how work is handed out, not what is computed)"""
    _, _, cpu, params = loaded
    cache = {}

    def get(frame, seed, split, method):
        key = (frame, seed, split, method)
        if key not in cache:
            cache[key] = cpu.render(O.camera_new(**params), options(frame, seed, split, method))
        return cache[key]
    return get


def options(frame, seed, split, method):
    o = abi.default_render_opts(frame[0], frame[1], 8, method=method, seed=seed)
    o.sample_split = split
    return o


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("seed", FRAME_SEEDS, ids=[hex(s) for s in FRAME_SEEDS])
@pytest.mark.parametrize("share", [0, 8])
@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("frame", FRAMES, ids=["72x40", "70x37"])
def test_rtweekend1_frames_are_the_oracles(hb, loaded, references, frame, split, share, seed, method):
    pair, general, _, params = loaded
    o = options(frame, seed, split, method)
    cam = hb.camera_new(**params)
    what = f"{frame[0]}x{frame[1]} split={split} share={share} seed={seed:#x} method={method}"
    for g in (pair, general):
        g.set_tuning(abi.RT_TUNE_WHOLE_PIXEL_SHARE, share)
    img, rays = pair.render(cam, o)
    info = pair.last_launch_info()
    assert "rt::FeatPair" in info["kernel"] and info["fine"] == 0, info
    # both frames are 9 x 5 tiles of 8 x 8: share 8 hands 22 of the 45 out as whole pixels when there are chunks
    assert info["whole_claims"] == (45 * share // 16 if split > 1 else 0), (what, info)
    img_g, rays_g = general.render(cam, o)
    assert "rt::Feat<false, false, false, false>" in general.last_launch_info()["kernel"], general.last_launch_info()
    ref, ref_rays = references(frame, seed, split, method)
    assert_images_match(img, ref, f"{what}: against the oracle")
    assert rays == ref_rays, (what, rays, ref_rays)
    assert_same_bits(img, img_g, f"{what}: against the general spheres-only kernel", nan_equal=False)
    assert rays == rays_g, (what, rays, rays_g)
