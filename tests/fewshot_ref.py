"""The few-shot memory-bank scoring restated in numpy: the definition the device is held to
(csrc/bank.hip: aaclip_bank_nn, aaclip_bank_distance, aaclip_fewshot_fuse).

The search and the combine step are stated in float64 on the operands as given (so on the rounded
16-bit operands when those are what the device reads); the fusion is stated in float32 with every
operation rounded once, which the device reproduces bit for bit.
"""
import numpy as np


def bank_nn(q, bank):
    """max_n q[m] . bank[n] in float64: [M]. q [M, K], bank [Nb, K], any float dtype."""
    q64, b64 = np.asarray(q, np.float64), np.asarray(bank, np.float64)
    out = np.full(q64.shape[0], -np.inf)
    # every dot product is its own sum over K (numpy's pairwise sum of one contiguous row), not a
    # BLAS call whose blocking depends on the shapes: the same bits wherever a row sits, so the
    # statement itself does not depend on the bank's order or on how it is cut into blocks
    step = max(1, (1 << 22) // (q64.shape[0] * q64.shape[1]))
    for n0 in range(0, b64.shape[0], step):
        sims = (q64[:, None, :] * b64[None, n0:n0 + step, :]).sum(axis=-1)
        out = np.maximum(out, sims.max(axis=1))
    return out


def bank_nn_parts(q, bank, n_splits, rows_per_split):
    """The per-split maxima, float64 [M, n_splits]: split s owns bank rows
    [s * rows_per_split, (s + 1) * rows_per_split)."""
    bank = np.asarray(bank)
    cols = [bank_nn(q, bank[s * rows_per_split:(s + 1) * rows_per_split]) for s in range(n_splits)]
    return np.stack(cols, axis=1)


def bank_distance(level_maxima):
    """sum over the levels of 1 - max similarity, float64 [M]. level_maxima: list of [M]."""
    return sum(1.0 - np.asarray(m, np.float64) for m in level_maxima)


def fewshot_grid(query_levels, bank_levels, batch, g):
    """The [B, 1, g, g] grid ahead of the blur, float64: row m = b * g * g + p."""
    d = bank_distance([bank_nn(q, r) for q, r in zip(query_levels, bank_levels)])
    return d.reshape(batch, 1, g, g)


def unit_range(x, lo, hi):
    """(x - lo) / (hi - lo) in float32, each operation rounded; 0 for a constant input."""
    x, lo, hi = np.asarray(x, np.float32), np.float32(lo), np.float32(hi)
    if not hi > lo:
        return np.zeros_like(x)
    return ((x - lo) / (hi - lo)).astype(np.float32)


def fewshot_fuse(zs_map, fs_map, zs_score):
    """(fused_map, fs_score, fused_score) in float32. zs_map / fs_map [n, ...], zs_score [n]; the
    ranges are the class's minimum and maximum of each of the four inputs."""
    zs_map, fs_map = np.asarray(zs_map, np.float32), np.asarray(fs_map, np.float32)
    zs_score = np.asarray(zs_score, np.float32).reshape(-1)
    fs_score = fs_map.reshape(fs_map.shape[0], -1).max(axis=1)
    fused_map = unit_range(zs_map, zs_map.min(), zs_map.max()) + unit_range(fs_map, fs_map.min(), fs_map.max())
    fused_score = (unit_range(zs_score, zs_score.min(), zs_score.max())
                   + unit_range(fs_score, fs_score.min(), fs_score.max()))
    return fused_map.astype(np.float32), fs_score.astype(np.float32), fused_score.astype(np.float32)
