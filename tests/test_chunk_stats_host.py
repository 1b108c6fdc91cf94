"""raytracing-rust_amd/csrc/rt_chunk_stats.h -- the one copy of what every reader of chunk sums computes (the demodulation divisors,
a chunk's luminance, (lbar, var) of a pixel, the state step in the form noise_chunk_kernel calls and in the form adaptive_fold_kernel
calls, and both maps to a pixel) -- run on the host by tests/cpp/chunk_stats_check.cpp and compared with noise_checker.estimate /
accumulate and with the accumulation inside adaptive_checker.adaptive by bit pattern (any NaN equals any NaN).  On the host the
operators are the plain IEEE ones, so this holds the arithmetic AS WRITTEN to the Python; what gfx950 computes with it the GPU suites
compare (test_gpu_noise.py, test_gpu_adaptive.py, test_gpu_adaptive_loop.py, test_gpu_robust.py).  A stand-alone program, its host
code built with AddressSanitizer and UBSan."""
import numpy as np
import pytest

import adaptive_checker as A
import host_check
import noise_checker as N

F32 = np.float32
H, W = 12, 25  # 300 pixels


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return host_check.build("chunk_stats_check", tmp_path_factory.mktemp("chunk_stats"), sanitize=True)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, F32).reshape(-1), np.ascontiguousarray(want, F32).reshape(-1)
    return bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def run_stats(exe, tmp_path, batch_sums, spp, albedo, masks=None, keep_state=True):
    """the program's planes after every batch: [(lbar, var, out_mean, out_lum, out_var)]; batch_sums[b] is (S, h, w, 3)"""
    split, h, w = batch_sums[0].shape[:3]
    n_px = h * w
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([n_px, split, spp // split, albedo is not None, keep_state, masks is not None, len(batch_sums)], np.uint32).tobytes())
        if albedo is not None:
            f.write(np.ascontiguousarray(albedo, F32).tobytes())
        for b, sums in enumerate(batch_sums):
            f.write(np.ascontiguousarray(sums, F32).tobytes())
            f.write(N.combine(sums, spp).astype(F32).tobytes())  # this render's mean, as the combine wrote it
            f.write((np.ones((h, w), np.uint32) if masks is None else masks[b].astype(np.uint32)).tobytes())
    host_check.run(exe, "stats", tmp_path / "in.bin", tmp_path / "out.bin", timeout=120)
    out = np.fromfile(tmp_path / "out.bin", F32).reshape(len(batch_sums), 7, h, w)
    return [(o[0], o[1], o[2:5].reshape(h, w, 3), o[5], o[6]) for o in out]  # (out_mean is [pixel][3]: 3 * h * w floats in a row)


def make_sums(rng, split):
    """(S, H, W, 3) chunk sums of either sign, none zero; pixel 0 has one NaN chunk, pixel 1 an infinite one, pixel 2 one of each"""
    sums = (rng.uniform(0.05, 4.0, (split, H, W, 3)) * rng.choice([-1.0, 1.0], (split, H, W, 3), p=[0.3, 0.7])).astype(F32)
    sums[split - 1, 0, 0, 1] = np.nan
    sums[0, 0, 1, 2] = np.inf
    sums[1, 0, 2, 0] = -np.inf
    sums[0, 0, 2, 1] = np.nan
    return sums


def make_albedo(rng):
    """components of 0, below 1e-3, exactly 1e-3 (the f32 the kernels clamp at) and NaN among ordinary ones"""
    albedo = rng.uniform(0.0, 1.0, (H, W, 3)).astype(F32)
    albedo[1, 0] = (0.0, 5e-4, 1e-3)
    albedo[1, 1] = (np.nan, 0.5, -0.0)
    albedo[1, 2] = (np.nextafter(F32(1e-3), F32(0)), np.nextafter(F32(1e-3), F32(1)), -1.0)
    albedo[0, 0, 0] = np.nan  # (under the pixel with the NaN chunk too)
    return albedo


@pytest.mark.parametrize("with_albedo", [False, True], ids=["no_albedo", "albedo"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("split", [2, 3, 64])
def test_a_fresh_sequence_and_two_added_batches_are_the_checkers_bits(exe, tmp_path, split, n, with_albedo):
    rng = np.random.default_rng(1000 * split + 10 * n + with_albedo)
    spp = split * n
    albedo = make_albedo(rng) if with_albedo else None
    batch_sums = [make_sums(rng, split) for _ in range(3)]
    got = run_stats(exe, tmp_path, batch_sums, spp, albedo)
    want_batches = [N.estimate(sums, spp, albedo) for sums in batch_sums]
    for b in range(3):
        lbar, var, out_mean, out_lum, out_var = got[b]
        assert same_bits(lbar, want_batches[b][1]) and same_bits(var, want_batches[b][2]), (b, "estimate")
        mean, lum_mean, variance = N.accumulate(want_batches[:b + 1])
        assert same_bits(out_mean, mean) and same_bits(out_lum, lum_mean) and same_bits(out_var, variance), (b, "state")
    # the cases are what they claim: the special pixels are special, the others finite
    assert np.isnan(got[0][0][0, 0]) and not np.isfinite(got[0][0][0, 1]) and np.isfinite(got[0][0][1:]).all()


def test_one_batch_without_a_state_writes_the_outputs_asked_for(exe, tmp_path):
    rng = np.random.default_rng(7)
    sums = make_sums(rng, 4)
    (lbar, var, out_mean, out_lum, out_var), = run_stats(exe, tmp_path, [sums], 8, None, keep_state=False)
    mean, want_lbar, want_var = N.estimate(sums, 8)
    assert same_bits(lbar, want_lbar) and same_bits(var, want_var)
    assert same_bits(out_mean, mean) and same_bits(out_lum, want_lbar)
    assert not out_var.any()  # the plane that was not asked for is not written


def test_per_pixel_batch_counts_are_the_adaptive_checkers_bits(exe, tmp_path):
    """adaptive_checker.adaptive on a 13 x 11 frame whose tile 0 is noise-free: it leaves the list after the first batch, so its
    pixels are divided by 1 and the others by 2 and 3; the program folds the batches adaptive() rendered, under its masks"""
    w, h, split, batch = 13, 11, 3, 6
    rng = np.random.default_rng(11)
    albedo = rng.uniform(0.2, 1.0, (h, w, 3)).astype(F32)
    still = rng.uniform(0.1, 1.0, (h, w, 3)).astype(F32)

    def batch_passes(b):
        p = np.random.default_rng(100 + b).uniform(0.0, 2.0, (batch, h, w, 3)).astype(F32)
        p[:, :8, :8] = still[:8, :8]
        return p
    want = A.adaptive(batch_passes, w, h, batch, split, 1, 3 * batch, threshold=1e-6, albedo=albedo)
    assert want["batches"] == 3 and [None if r is None else list(r) for r in want["rendered"]] == [None, [1, 2, 3], [1, 2, 3]]
    masks = [np.ones((h, w), bool)] + [A.tile_mask(r, w, h) for r in want["rendered"][1:]]
    got = run_stats(exe, tmp_path, [N.chunk_sums(batch_passes(b), split) for b in range(3)], batch, albedo, masks=masks)
    lbar, var, out_mean, out_lum, out_var = got[-1]
    assert same_bits(out_mean, want["mean"]) and same_bits(out_lum, want["lum_mean"]) and same_bits(out_var, want["variance"])
    assert sorted(set((want["passes"] // batch).reshape(-1).tolist())) == [1, 3]


def test_both_maps_to_a_pixel(exe, tmp_path):
    w, h, tile_w, tile_h = 13, 11, 4, 16
    host_check.run(exe, "maps", w, h, tile_w, tile_h, tmp_path / "maps.bin", timeout=120)
    v = np.fromfile(tmp_path / "maps.bin", np.int32)
    tx, ty = (w + 7) // 8, (h + 7) // 8
    grid, work = v[:tx * ty * 64 * 3].reshape(tx * ty, 64, 3), v[tx * ty * 64 * 3:]
    for t in range(tx * ty):
        inside, x, y = grid[t, :, 0].astype(bool), grid[t, :, 1], grid[t, :, 2]
        # place j = 8 * (y & 7) + (x & 7) of its tile (noise_checker.tile_slots), in the tile adaptive_checker.tile_mask lists
        assert (8 * (y & 7) + (x & 7) == np.arange(64)).all() and (x // 8 == t % tx).all() and (y // 8 == t // tx).all()
        mask = np.zeros((h, w), bool)
        mask[y[inside], x[inside]] = True
        assert (mask == A.tile_mask([t], w, h)).all() and inside.sum() == mask.sum()
        assert ((x < w) & (y < h) == inside).all()
    # the render's work order: tiles row-major, pixels row-major inside a tile, padding of edge tiles counted
    ax, ay = (w + tile_w - 1) // tile_w, (h + tile_h - 1) // tile_h
    padded = np.full((ay * tile_h, ax * tile_w), -1, np.int64)
    padded[:h, :w] = np.arange(h * w).reshape(h, w)
    want = padded.reshape(ay, tile_h, ax, tile_w).transpose(0, 2, 1, 3).reshape(-1)
    assert work.size == want.size and (work == want).all()
