"""The noise estimates of include/rt_hip.h (rt_noise_opts) restated in numpy float32, written from the header text.  Every operation
is one IEEE f32 operation on arrays (numpy rounds each to f32, as the kernels do with contraction off), sums run left to right
from +0 and the tile sum is the header's butterfly, so the GPU is held to these functions bit for bit (tests/test_gpu_noise.py).

The per-pass images come from the CPU oracle: a render of ONE pass (samples_per_pixel 1, sample_begin s, sample_split 1) returns
pass s exactly -- a running mean over one pass is the pass.  Chunk sums, the combine and everything after are restated here."""
import numpy as np

F32 = np.float32
TILE = 8


def lum(e):
    """the denoiser's lum, f32, left to right"""
    return (F32(0.2126) * e[..., 0] + F32(0.7152) * e[..., 1]) + F32(0.0722) * e[..., 2]


def passes(cpu_scene, cpu_camera, opts, n_passes, sample_begin=None):
    """(n_passes, H, W, 3) f32: passes [sample_begin, sample_begin + n_passes) of a render under `opts` (an abi.RenderOpts; its
    samples_per_pixel, sample_begin unless given, and sample_split are not used)"""
    import copy
    o = copy.copy(opts)
    begin = int(opts.sample_begin if sample_begin is None else sample_begin)
    o.samples_per_pixel, o.sample_split = 1, 1
    out = np.zeros((n_passes, opts.height, opts.width, 3), F32)
    for s in range(n_passes):
        o.sample_begin = (begin + s) & ((1 << 64) - 1)  # a uint64_t addition: it wraps (rt_render_opts.sample_begin)
        out[s] = cpu_scene.render(cpu_camera, o, n_threads=1)[0]
    return out


def chunk_bounds(spp, split):
    """[b_0 .. b_S]: chunk c holds passes [b_c, b_c+1) = [floor(c*spp/S), floor((c+1)*spp/S)), the rule of
    rt_render_opts.sample_split.  Where S divides spp these are the equal chunks [c*n, (c+1)*n), n = spp / S."""
    assert 1 <= split <= spp, (spp, split)
    return [(c * spp) // split for c in range(split + 1)]


def chunk_sums(pass_images, split, bounds=None):
    """(S, H, W, 3): chunk c = passes [b_c, b_c+1) summed in pass order from +0; the bounds are chunk_bounds' unless given"""
    spp = len(pass_images)
    b = chunk_bounds(spp, split) if bounds is None else list(bounds)
    assert len(b) == split + 1 and b[0] == 0 and b[-1] == spp and all(lo <= hi for lo, hi in zip(b, b[1:])), (spp, split, b)
    sums = np.zeros((split,) + pass_images.shape[1:], F32)
    for c in range(split):
        for s in range(b[c], b[c + 1]):
            sums[c] = sums[c] + pass_images[s]
    return sums


def combine(sums, spp):
    """what rt_render writes at sample_split = S: the chunk sums added in chunk order from +0, divided by spp once"""
    acc = np.zeros(sums.shape[1:], F32)
    for c in range(len(sums)):
        acc = acc + sums[c]
    return acc / F32(spp)


def estimate(sums, spp, albedo=None):
    """(mean (H, W, 3), lbar (H, W), var (H, W)) of one render from its chunk sums"""
    split = len(sums)
    assert split >= 2 and spp % split == 0, (spp, split)
    n = F32(spp // split)
    d = np.fmax(np.asarray(albedo, F32), F32(1e-3)) if albedo is not None else np.ones(sums.shape[1:], F32)
    with np.errstate(all="ignore"):
        l = [lum(sums[c] / n / d) for c in range(split)]
        lsum = np.zeros(sums.shape[1:3], F32)
        for c in range(split):
            lsum = lsum + l[c]
        lbar = lsum / F32(split)
        sq = np.zeros(sums.shape[1:3], F32)
        for c in range(split):
            dl = l[c] - lbar
            sq = sq + dl * dl
        var = sq / F32(split * (split - 1))
        return combine(sums, spp), lbar.astype(F32), var.astype(F32)


def accumulate(batches):
    """(mean, lum_mean, variance) after the (mean_b, lbar_b, var_b) of `batches`, in order"""
    m, l, v = (np.zeros_like(x) for x in batches[0])
    for mean_b, lbar_b, var_b in batches:
        m, l, v = m + mean_b, l + lbar_b, v + var_b
    nb = F32(len(batches))
    with np.errstate(all="ignore"):
        return m / nb, l / nb, v / (nb * nb)


def tile_slots(lum_mean, variance, luminance_floor):
    """(tiles_y, tiles_x, 64) f32: slot j = 8 * (y & 7) + (x & 7) of every tile holds the pixel's r, slots outside the frame +0;
    and the number of pixels of each tile inside the frame"""
    lum_mean, variance = np.asarray(lum_mean, F32), np.asarray(variance, F32)
    h, w = lum_mean.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    with np.errstate(all="ignore"):
        r = np.sqrt(variance) / (np.abs(lum_mean) + F32(luminance_floor))
    r = np.where(np.isfinite(r), r, F32(np.inf)).astype(F32)
    padded = np.zeros((ty * TILE, tx * TILE), F32)
    padded[:h, :w] = r
    inside = np.zeros((ty * TILE, tx * TILE), np.int64)
    inside[:h, :w] = 1
    slots = padded.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE)
    count = inside.reshape(ty, TILE, tx, TILE).sum(axis=(1, 3))
    return slots, count


def tiles(lum_mean, variance, luminance_floor=0.01, threshold=0.05):
    """(tile_error (tiles_y, tiles_x) f32, summary dict)"""
    v, count = tile_slots(lum_mean, variance, luminance_floor)
    idx = np.arange(TILE * TILE)
    with np.errstate(all="ignore"):
        for k in range(6):
            v = v + v[..., idx ^ (1 << k)]
    assert (v == v[..., :1]).all() or np.isnan(v).any()  # every slot ends with the same value
    err = (v[..., 0] / count.astype(F32)).astype(F32)
    summary = {"max_tile_error": F32((err + F32(0.0)).max()), "tiles_above": int((err > F32(threshold)).sum()), "n_tiles": int(err.size)}
    return err, summary


def render_estimate(cpu_scene, cpu_camera, opts, split, albedo=None, sample_begin=None, n_passes=None):
    """{"mean", "lum_mean", "variance"} of ONE render of opts.samples_per_pixel passes at sample_split = split"""
    spp = int(opts.samples_per_pixel if n_passes is None else n_passes)
    sums = chunk_sums(passes(cpu_scene, cpu_camera, opts, spp, sample_begin), split)
    return estimate(sums, spp, albedo)
