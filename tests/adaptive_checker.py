"""rt_render_adaptive restated in numpy f32 (include/rt_hip.h): the loop of noise_checker's pieces -- `chunk_sums`, `estimate`,
`tiles` -- with a batch count per pixel.  Nothing new is computed here but the division by the pixel's own count and the
selection of the active tiles; the per-pass images come from the caller (the CPU oracle through noise_checker.passes, or a hand
case)."""
import numpy as np

import noise_checker as N

F32 = np.float32
TILE = 8


def select(tile_error, threshold):
    """ascending indices of the tiles with error > threshold (strictly; NaN is not above)"""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.asarray(tile_error, F32).reshape(-1) > F32(threshold)).astype(np.uint32)


def tile_mask(tiles, w, h):
    """(h, w) bool: the pixels of the listed tiles"""
    tx = (w + TILE - 1) // TILE
    m = np.zeros((h, w), bool)
    for t in tiles:
        y, x = TILE * (int(t) // tx), TILE * (int(t) % tx)
        m[y:y + TILE, x:x + TILE] = True
    return m


def adaptive(batch_passes, w, h, batch, split, min_batches, max_passes, luminance_floor=0.01, threshold=0.05, albedo=None):
    """batch_passes(b) -> (batch, h, w, 3) f32, the passes of window b.  Returns the outputs of rt_render_adaptive and, per batch,
    the list that was rendered (`rendered`, None = the whole frame by rule) and the list selected after it (`active`)."""
    n_tiles = ((w + TILE - 1) // TILE) * ((h + TILE - 1) // TILE)
    M, L, V = np.zeros((h, w, 3), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
    nb = np.zeros((h, w), np.uint32)
    active = np.arange(n_tiles, dtype=np.uint32)  # before any batch every tile is active
    rendered, selected, states = [], [], []
    b = 0
    while True:
        whole = b < min_batches
        mask = np.ones((h, w), bool) if whole else tile_mask(active, w, h)
        rendered.append(None if whole else active.copy())
        mean_b, lbar_b, var_b = N.estimate(N.chunk_sums(np.asarray(batch_passes(b), F32), split), batch, albedo)
        M[mask] = (M + mean_b)[mask]
        L[mask] = (L + lbar_b)[mask]
        V[mask] = (V + var_b)[mask]
        nb[mask] += 1
        nf = nb.astype(F32)
        mean, lum_mean, variance = M / nf[..., None], L / nf, V / (nf * nf)
        tile_error, summary = N.tiles(lum_mean, variance, luminance_floor, threshold)
        active = select(tile_error, threshold)
        selected.append(active.copy())
        states.append(tile_error.copy())
        b += 1
        converged = b >= min_batches and len(active) == 0
        if converged or (b + 1) * batch > max_passes:
            break
    passes = nb * np.uint32(batch)
    return {"mean": mean, "lum_mean": lum_mean, "variance": variance, "tile_error": tile_error, "passes": passes, "batches": b,
            "converged": bool(converged), "pixel_passes": int(passes.astype(np.uint64).sum()), "summary": summary,
            "rendered": rendered, "active": selected, "tile_errors": states}
