"""Greedy k-centre coreset selection restated in numpy float64: the definition the device is held
to (csrc/bank.hip: aaclip_bank_coreset).

Farthest-point selection under the distance 1 - cosine on unit rows: from `start`, pick m - 1 times
the row whose largest similarity to the rows picked so far is smallest, the lowest index on ties.
Rows are taken as given (normalising them is the caller's job, as it is for fewshot_ref.bank_nn).
"""
import numpy as np


def row_sims(rows64, c):
    """rows64 @ rows64[c] with every dot product its own sum over K (numpy's pairwise sum of one
    contiguous row, as in fewshot_ref.bank_nn), not a BLAS call whose blocking depends on the shape:
    a row's similarity has the same bits wherever the row sits."""
    out = np.empty(rows64.shape[0])
    step = max(1, (1 << 22) // rows64.shape[1])
    for n0 in range(0, rows64.shape[0], step):
        out[n0:n0 + step] = (rows64[n0:n0 + step] * rows64[c][None, :]).sum(axis=-1)
    return out


def greedy_kcenter(rows, m, start=0):
    """(sel [m] int64, cover [m] float64, maxsim [N] float64). rows [N, K] of any float dtype,
    1 <= m <= N, 0 <= start < N. sel[0] = start, cover[0] = -inf; cover[t] is pick t's largest
    similarity to the picks before it; maxsim[n] the largest similarity of row n to any pick."""
    r = np.ascontiguousarray(np.asarray(rows, np.float64))
    n = r.shape[0]
    if not (1 <= m <= n and 0 <= start < n):
        raise ValueError(f"need 1 <= m <= N and 0 <= start < N, got m = {m}, start = {start}, N = {n}")
    maxsim = np.full(n, -np.inf)
    taken = np.zeros(n, bool)
    sel = np.empty(m, np.int64)
    cover = np.empty(m)
    sel[0], cover[0] = start, -np.inf
    for t in range(m):
        c = sel[t]
        taken[c] = True
        maxsim = np.maximum(maxsim, row_sims(r, c))  # every row, taken ones included
        if t == m - 1:
            break
        key = np.where(taken, np.inf, maxsim)
        sel[t + 1] = int(np.argmin(key))  # argmin: the lowest index attaining the minimum
        cover[t + 1] = key[sel[t + 1]]
    return sel, cover, maxsim


def maxsim_over(rows, sel):
    """max over s in sel of rows[n] . rows[s], float64 [N]."""
    r = np.ascontiguousarray(np.asarray(rows, np.float64))
    out = np.full(r.shape[0], -np.inf)
    for c in sel:
        out = np.maximum(out, row_sims(r, int(c)))
    return out
