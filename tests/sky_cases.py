"""The sky tables the kernels treat differently, as ONE table: test_sky_tables.py (CPU) shows through the host-only build that every
case is in the regime it is there for, test_gpu_sky.py runs the kernels' sky code (rt_selftest_sky) and renders on it.  A case is a
sky texture, a sampler_res and what the host must make of them: the guide width, whether the tables may be staged in LDS (the
96 KB rule of csrc/rt_api_internal.h) and whether sky_sample divides by the resolutions through verified reciprocals (recorded from
rt_selftest_division on both axes; the CPU file asserts the record).  torch is never imported here."""
import functools

import numpy as np

import scenes

abi = scenes.abi
F32 = np.float32
LDS_LIMIT = 96 * 1024
# the self-test's streams.  The seed is the smallest at which the oracle's draws reach min(cells, 1000) distinct cells on every
# monotone case (searched on the CPU, oracle only: the six pole cells of `k256_tall` expect 0.8 of the 65 536 draws each)
SELFTEST_N, SELFTEST_SEED = 65536, 84
# ties (a draw k * 2^-24 that equals a CDF entry): the samples test_sky_tables.py counts them over and test_gpu_sky.py runs
TIE_N, TIE_SEED = 1 << 21, 11
TIE_CASES = ("k256_wide", "unguided_wide")  # one guided, one unguided: rows of 255 and 256 entries
# renders: 32 x 18, 8 passes, MIS
W, H, SPP, SEED = 32, 18, 8, 3

LERP = ((0.5, 0.7, 1.0), (1.0, 1.0, 1.0))  # the sky of tests/scenes.py
# Lerp towards a colour whose green is far below zero: the luminance of the lower rows is negative, the upper rows' positive,
# so the marginal CDF rises and falls
NEGATIVE = ((0.5, 0.7, 1.0), (1.0, -3.0, 1.0))


def plateau_image():
    """9 x 17 texels.  An image texture looks a direction up in (height - 1) x (width - 1) = 8 x 16 texels (textures/mod.rs:232-262),
    so each cell of a 32 x 16 sampler lies inside one texel: two cells by two.  Texel row 3 is zero, and so is every texel with
    (2 x + 3 y) % 4 == 0: 48 of the 128 texels the sampler sees, about a third."""
    y, x = np.mgrid[0:9, 0:17]
    value = (0.25 + ((3 * x + 5 * y) % 7) / 8.0).astype(F32)
    value[(2 * x + 3 * y) % 4 == 0] = 0.0
    value[3, :] = 0.0
    return np.repeat(value[:, :, None], 3, axis=2) * np.array([1.0, 0.9, 0.8], dtype=F32)


class Case:
    """texture(sc) -> texture index; res = sampler_res; guide_k, fits_lds, inv_res_ok: what the host must report; monotone: every CDF
    is finite and non-decreasing; one_cell_only: the reason why every draw lands in the same cell (else None)"""

    def __init__(self, texture, res, guide_k, inv_res_ok, fits_lds=True, monotone=True, one_cell_only=None, what=""):
        self.texture, self.res, self.guide_k, self.inv_res_ok = texture, res, guide_k, inv_res_ok
        self.fits_lds, self.monotone, self.one_cell_only, self.what = fits_lds, monotone, one_cell_only, what


def _lerp(colours):
    return lambda sc: sc.lerp(*colours)


CASES = {
    "control": Case(_lerp(LERP), (16, 8), 16, 1, what="the regime the suite already covers"),
    "k256_wide": Case(_lerp(LERP), (254, 3), 256, 1, what="guide_k 256, byte entry 255"),
    "k256_tall": Case(_lerp(LERP), (3, 254), 256, 1, what="the same on the marginal"),
    "unguided_wide": Case(_lerp(LERP), (255, 4), 0, 1, what="binary search, small tables"),
    "unguided_tall": Case(_lerp(LERP), (4, 255), 0, 1, what="binary search on the marginal"),
    "big_guided": Case(_lerp(LERP), (200, 120), 256, 1, fits_lds=False, what="127 940 bytes with guides: over the LDS limit, guided"),
    "big_unguided": Case(_lerp(LERP), (300, 200), 0, 1, fits_lds=False, what="241 604 bytes, no guide"),
    "plateaus": Case(lambda sc: sc.image(plateau_image()), (32, 16), 32, 1, what="zero-pdf cells, repeated CDF entries, zero-sum rows"),
    "negative": Case(_lerp(NEGATIVE), (16, 8), 0, 1, monotone=False, what="non-monotone CDF: the guide is refused at a small size"),
    "black": Case(lambda sc: sc.solid((0.0, 0.0, 0.0)), (16, 8), 16, 1, what="all-zero tables (c == 0: not normalised)",
                  one_cell_only="every entry of every CDF is 0 <= any draw: each search runs off the end and is clamped to the last cell"),
    "one_cell": Case(_lerp(LERP), (1, 1), 16, 1, what="degenerate tables"),
    "one_row": Case(_lerp(LERP), (32, 1), 32, 1, what="degenerate tables"),
    "one_column": Case(_lerp(LERP), (1, 32), 32, 1, what="degenerate tables"),
    # The plain division u = nu / res_x.  rt_selftest_division verifies the reciprocal of every integer from 1 to 6000, and of
    # 2^24 - 1 (the one significand of all ones below 2^24), so no small table takes that form; the library verifies nothing for a
    # resolution of 2^24 or more (csrc/rt_api.cpp sky_reciprocals).  These are the two smallest such tables: one row of 64 MB.
    "huge_row": Case(_lerp(LERP), (1 << 24, 1), 0, 0, fits_lds=False, what="plain division: 2^24 cells in one row"),
    "huge_row_next": Case(_lerp(LERP), ((1 << 24) + 2, 1), 0, 0, fits_lds=False, what="plain division: the next resolution a float holds"),
}
BIG = ("big_guided", "big_unguided")
HUGE = ("huge_row", "huge_row_next")
VERIFIED_BELOW = 1 << 24  # resolutions the library tries to verify a reciprocal for


def table_bytes(rx, ry, guide_k):
    """CDFs and guides: what the host (csrc/rt_api_internal.h sky_table_bytes) compares with its limit for tables in LDS"""
    return (ry * (rx + 1) + ry + 1) * 4 + (ry + 1) * guide_k


def with_sky(sc, name):
    """`sc` with the sky of case `name` in place of its own (the texture and its Emit material are appended: no index of the
    scene moves)"""
    case = CASES[name]
    sc.set_sky(case.texture(sc), case.res)
    return sc


def unsampled(sc, name):
    """the same sky texture with sampler_res (0, 0): what a NAIVE render of the case must equal"""
    sc.set_sky(CASES[name].texture(sc), (0, 0))
    return sc


def sky_only(name):
    """one small sphere under the case's sky: the scene of the table and self-test checks"""
    sc = scenes.SceneDescription()
    sc.sphere((0, 0, -3), 1.0, sc.lambertian(sc.solid(0.5), 0.5))
    return with_sky(sc, name)


FLOOR_CAMERA = dict(origin=(0.0, -6.0, 2.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 0.0, 1.0), fov=60.0,
                    aspect_ratio=float(F32(16.0) / F32(9.0)), aperture=0.0, focus_dist=10.0)
# one scene per feature set of the render kernels: (scene without the case's sky, camera parameters)
RENDER_SCENES = {
    "floor": lambda: (scenes.floor_under(sky=LERP, sampler_res=(16, 8)), FLOOR_CAMERA),
    "spheres": lambda: (scenes.random_spheres(30, seed=5), scenes.TINY_TREE_CAMERA),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
}
RENDER_CASES = tuple(name for name in CASES if name != "negative")  # an integrator fed negative pdfs has no defined result


def _neighbours(a):
    a = np.asarray(a, dtype=F32)
    return np.concatenate([a, np.nextafter(a, F32(-np.inf)), np.nextafter(a, F32(np.inf))])


@functools.lru_cache(maxsize=None)
def chosen_directions(name):
    """[m, 3] float32: where sky_pdf can go wrong whatever the table (poles, axes, signed zeros, the phi seam, a zero, an
    unnormalised, a NaN and an infinite vector), then every cell corner of the case's table -- theta = pi j / res_y, phi =
    2 pi i / res_x in float64, rounded once to f32 -- with its two f32 neighbours in theta and in phi (the big cases: the first,
    middle and last row and column; the huge ones: those columns of their one row)"""
    tiny, sub = np.finfo(F32).tiny, F32(1e-45)
    nan, inf = F32(np.nan), F32(np.inf)
    fixed = []
    for s in (1.0, -1.0):
        for axis in range(3):
            for zero in (0.0, -0.0):
                d = [zero, zero, zero]
                d[axis] = s
                fixed.append(d)
    for x in (1.0, -1.0):
        for y in (tiny, -tiny, sub, -sub, 0.0, -0.0):
            fixed.append([x, y, 0.0])
            fixed.append([x * 0.6, y, 0.8])
    fixed += [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [3.0, -4.0, 12.0], [0.1, 0.2, 0.05], [nan, 0.5, 0.5], [0.5, nan, 0.5], [0.5, 0.5, nan],
              [inf, 0.0, 0.0], [0.0, -inf, 0.5], [0.3, 0.4, inf]]
    fixed = np.array(fixed, dtype=F32)
    rx, ry = CASES[name].res
    i, j = (None if name in HUGE else np.arange(rx + 1)), np.arange(ry + 1)
    if name in BIG:
        i, j = np.array([0, 1, rx // 2, rx - 1, rx]), np.array([0, 1, ry // 2, ry - 1, ry])
        # (the corners of the first, middle and last column with every row, and of those rows with every column)
        pairs = np.concatenate([np.stack(np.meshgrid(i, np.arange(ry + 1), indexing="ij"), -1).reshape(-1, 2),
                                np.stack(np.meshgrid(np.arange(rx + 1), j, indexing="ij"), -1).reshape(-1, 2)])
    elif name in HUGE:  # (one row: its two edges at the first, second, middle and last columns)
        pairs = np.stack(np.meshgrid(np.array([0, 1, rx // 2, rx - 1, rx]), j, indexing="ij"), -1).reshape(-1, 2)
    else:
        pairs = np.stack(np.meshgrid(i, j, indexing="ij"), -1).reshape(-1, 2)
    phi = (2.0 * np.pi * pairs[:, 0].astype(np.float64) / rx).astype(F32)
    theta = (np.pi * pairs[:, 1].astype(np.float64) / ry).astype(F32)
    # both angles' neighbours, one at a time and together
    phi3, theta3 = _neighbours(phi).reshape(3, -1), _neighbours(theta).reshape(3, -1)
    ph = np.concatenate([phi3[a] for a in range(3) for b in range(3)]).astype(np.float64)
    th = np.concatenate([theta3[b] for a in range(3) for b in range(3)]).astype(np.float64)
    corners = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1).astype(F32)
    out = np.ascontiguousarray(np.concatenate([fixed, corners]))
    out.setflags(write=False)
    return out


# ---- the three searches of test_sky_tables.py, vectorised over draws ----
def search_reference(cdf, num):
    """the reference's binary search for the upper bound (distributions.rs:51-72, csrc/rt_shade.h dist1d_sample without a guide),
    clamped to a cell index; cdf has n + 1 entries"""
    cdf = np.asarray(cdf, dtype=F32)
    n = cdf.size - 1
    first = np.zeros(num.shape, dtype=np.int64)
    length = np.full(num.shape, n + 1, dtype=np.int64)
    while (length > 0).any():
        live = length > 0
        half = length >> 1
        middle = np.minimum(first + half, n)  # (dead lanes only: a live lane's middle is inside the table)
        le = live & (cdf[middle] <= num)
        gt = live & ~le
        first = np.where(le, middle + 1, first)
        length = np.where(le, length - (half + 1), np.where(gt, half, length))
    return np.minimum(first - 1, n - 1)


def search_guided(cdf, guide_row, num):
    """the kernels' guided scan (csrc/rt_shade.h dist1d_sample): start at guide[(uint)(num * K)], step right two entries per round"""
    cdf = np.asarray(cdf, dtype=F32)
    n = cdf.size - 1
    k = guide_row.size
    first = guide_row[(num * F32(k)).astype(np.uint32)].astype(np.int64)
    live = np.ones(num.shape, dtype=bool)
    while live.any():
        c0, c1 = cdf[np.minimum(first, n)], cdf[np.minimum(first + 1, n)]
        b0 = live & (first <= n) & (c0 <= num)
        b1 = b0 & (first + 1 <= n) & (c1 <= num)
        first = first + b0 + b1
        live = b1
    return np.minimum(first - 1, n - 1)


def search_numpy(cdf, num):
    cdf = np.asarray(cdf, dtype=F32)
    return np.minimum(np.searchsorted(cdf, num, side="right").astype(np.int64) - 1, cdf.size - 2)


def all_draws(lo, hi):
    """the draws k * 2^-24, lo <= k < hi (rt_rng_f32: exact in float32)"""
    return (np.arange(lo, hi, dtype=np.uint32).astype(F32) * F32(2.0 ** -24)).astype(F32)
