"""Tiled inference in numpy: the plan, the gather, the stitch, the global-view blend and the score
of include/aaclip.h (csrc/tiles.hip), in float64.

plan() builds the per-axis tables from the stated integer formulas, every weight computed in
float64 and rounded once to float32: the values aaclip_tile_plan must return exactly. stitch()
and score() read those float32 tables (and the float32 coefficients a, 1 - a) and do everything
else in float64, so what separates them from the kernel is the kernel's own fp32 products and sums.
"""
import numpy as np


def canvas_side(S, G, O):
    return G * S - (G - 1) * O


def ramp(S, G, O, i, u):
    """1-D blend weight of tile i at local coordinate u (float64)."""
    if i > 0 and u < O:
        return (u + 0.5) / O
    if i < G - 1 and u >= S - O:
        return (S - u - 0.5) / O
    return 1.0


def plan(S, G, O, dtype=np.float32):
    """(index int32 [C, 2] = first covering tile, i0; weight float32 [C, 4] = the first tile's
    weight, the next tile's or 0, 1 - lambda, lambda). dtype=np.float64 keeps the weights
    unrounded (what the formulas give before the table's one rounding)."""
    assert 2 <= G <= 8 and 0 <= 2 * O <= S
    C, step = canvas_side(S, G, O), S - O
    index, weight = np.zeros((C, 2), np.int32), np.zeros((C, 4), dtype)
    for c in range(C):
        cover = [i for i in range(G) if i * step <= c < i * step + S]
        assert 1 <= len(cover) <= 2 and cover == list(range(cover[0], cover[0] + len(cover)))
        index[c, 0] = cover[0]
        w = [ramp(S, G, O, i, c - i * step) for i in cover]
        weight[c, 0] = w[0]
        weight[c, 1] = w[1] if len(w) == 2 else 0.0
        num, den = (2 * c + 1) * S - C, 2 * C
        i0, rem = (0, 0) if num < 0 else divmod(num, den)
        index[c, 1] = i0
        weight[c, 2] = (den - rem) / den
        weight[c, 3] = rem / den
    return index, weight


def gather(canvas, S, G, O):
    """canvas [n, 3, C, C] -> tiles [n G^2, 3, S, S], image-major, t = ty G + tx."""
    step = S - O
    return np.stack([canvas[b, :, ty * step:ty * step + S, tx * step:tx * step + S]
                     for b in range(canvas.shape[0]) for ty in range(G) for tx in range(G)])


def _axis_matrix(index, weight, S, G, O):
    """[C, G S] float64: row c holds tile i's weight at column i S + (c - origin_i)."""
    C, step = index.shape[0], S - O
    A = np.zeros((C, G * S))
    for c in range(C):
        f = int(index[c, 0])
        A[c, f * S + c - f * step] = float(weight[c, 0])
        if weight[c, 1] != 0:
            A[c, (f + 1) * S + c - (f + 1) * step] = float(weight[c, 1])
    return A


def _bilinear_matrix(index, weight, S):
    C = index.shape[0]
    L = np.zeros((C, S))
    for c in range(C):
        i0 = int(index[c, 1])
        L[c, i0] += float(weight[c, 2])
        L[c, min(i0 + 1, S - 1)] += float(weight[c, 3])
    return L


def upsample(global_maps, index, weight):
    """The global maps [B, S, S] on the canvas [B, C, C]: bilinear, half-pixel centres (float64)."""
    L = _bilinear_matrix(index, weight, global_maps.shape[-1])
    return L @ global_maps.astype(np.float64) @ L.T


def coefficients(global_weight):
    """(1 - a, a) as the kernel holds them: a in float32, 1 - a one float32 subtraction."""
    a = np.float32(global_weight)
    return float(np.float32(1) - a), float(a)


def stitch(tile_maps, S, G, O, tables, global_maps=None, global_weight=0.0):
    """tile_maps [B G^2, S, S] (+ global_maps [B, S, S]) -> [B, C, C] float64, from the float32
    tables = (index, weight)."""
    index, weight = tables
    B = tile_maps.shape[0] // (G * G)
    A = _axis_matrix(index, weight, S, G, O)
    t = tile_maps.astype(np.float64).reshape(B, G, G, S, S).transpose(0, 1, 3, 2, 4).reshape(B, G * S, G * S)
    out = A @ t @ A.T
    keep, a = coefficients(global_weight)
    if a == 0.0:
        return out
    return keep * out + a * upsample(global_maps, index, weight)


def score(tile_scores, G, global_scores=None, global_weight=0.0):
    m = tile_scores.astype(np.float64).reshape(-1, G * G).max(axis=1)
    keep, a = coefficients(global_weight)
    if a == 0.0:
        return m
    return keep * m + a * global_scores.astype(np.float64)
