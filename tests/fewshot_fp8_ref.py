"""Reference statement of the MX fp8 few-shot search (csrc/rows.hip aaclip_unit_rows_fp8mx, csrc/bank.hip
aaclip_bank_nn_fp8mx) in numpy. The storage format is csrc/mxfp8.h's:

  * values OCP e4m3, one byte each; 64 consecutive columns of a row share one e8m0 byte e + 127;
  * e = the smallest integer with amax * 2^-e <= 448, clamped to [-126, 127], 0 for an all-zero block;
  * a value is stored as RNE_e4m3(x * 2^-e): the scaling is exact, the conversion the only rounding
    (torch's CPU float8_e4m3fn cast is that conversion);
  * scale buffer [cols / 128][ld][2].

The search returns the cosine between the STORED rows: with deq = e4m3 * 2^e,
cos[m, n] = deq_q[m] . deq_r[n] / (|deq_q[m]| |deq_r[n]|), 0 where a row stores all zeros."""
import numpy as np
import torch

import fewshot_ref as FR

BLOCK = 64


def mx_exponents(x):
    """e [rows, cols / 64] int64 of x [rows, cols] (float32 values: the rule is applied to what the
    device holds)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    rows, cols = x.shape
    amax = np.abs(x).reshape(rows, cols // BLOCK, BLOCK).max(axis=-1)
    _, ex = np.frexp(amax)  # amax = m 2^ex, m in [0.5, 1)
    e = ex.astype(np.int64) - 9  # amax 2^-e in [256, 512)
    e = e + (np.ldexp(amax, -e) > 448.0)
    return np.where(amax > 0, np.clip(e, -126, 127), 0)


def e4m3_rne(x):
    """float -> e4m3 codes (uint8), round to nearest even; x must already be fp32-exact."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def e4m3_values(codes):
    """e4m3 codes (uint8) -> float64."""
    t = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8))
    return t.view(torch.float8_e4m3fn).to(torch.float64).numpy()


def mx_quantise(x):
    """x [rows, cols] float32 -> (codes uint8 [rows, cols], e int64 [rows, cols / 64])."""
    x = np.asarray(x, np.float32)
    e = mx_exponents(x)
    scaled = np.ldexp(x.astype(np.float64), -np.repeat(e, BLOCK, axis=1))  # exact: a power of two
    return e4m3_rne(scaled), e


def scale_buffer(e, ld=None):
    """e [rows, cols / 64] -> the device's scale buffer uint8 [cols / 128, ld, 2] (rows past the end 0)."""
    rows, nblk = e.shape
    ld = ld or (rows + 1) // 2 * 2
    sc = np.zeros((nblk // 2, ld, 2), np.uint8)
    sc[:, :rows, :] = (e + 127).astype(np.uint8).reshape(rows, nblk // 2, 2).transpose(1, 0, 2)
    return sc


def exponents_of(sc, rows):
    """The device's scale buffer [cols / 128, ld, 2] -> e int64 [rows, cols / 64]."""
    sc = np.asarray(sc)
    return sc[:, :rows, :].transpose(1, 0, 2).reshape(rows, -1).astype(np.int64) - 127


def dequantise(codes, sc):
    """The device's (q, sc) buffers -> float64 [rows, cols]: e4m3 * 2^e, what the search reads."""
    codes = np.asarray(codes)
    e = exponents_of(sc, codes.shape[0])
    return np.ldexp(e4m3_values(codes), np.repeat(e, BLOCK, axis=1))


def unit_rows(x):
    """aaclip_unit_rows_fp8mx on rows whose fp32 normalisation is exact (designed rows: the norm is a
    power of two) or close enough not to matter to the caller: (codes, e, rnorm float32). rnorm in
    float64 then rounded: exact where the stored norm is a power of two."""
    x = np.asarray(x, np.float64)
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    y = (x / np.maximum(norm, 1e-12)).astype(np.float32)
    codes, e = mx_quantise(y)
    deq = np.ldexp(e4m3_values(codes), np.repeat(e, BLOCK, axis=1))
    ss = (deq * deq).sum(axis=1)
    rnorm = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0).astype(np.float32)
    return codes, e, rnorm


def stored_unit(deq):
    """deq [rows, cols] float64 -> the rows over their norms (all-zero rows stay zero): the cosine
    between stored rows is the dot product of these."""
    n = np.sqrt((deq * deq).sum(axis=1, keepdims=True))
    return np.where(n > 0, deq / np.where(n > 0, n, 1.0), 0.0)


def cosines(deq_q, deq_r):
    """The full [M, Nb] cosine matrix of the stored rows, float64."""
    return stored_unit(deq_q) @ stored_unit(deq_r).T


def bank_nn_parts(deq_q, deq_r, n_splits, rows_per_split):
    """part [M, n_splits]: per split of the bank rows the largest cosine (fewshot_ref.bank_nn_parts on
    the stored rows over their norms)."""
    return FR.bank_nn_parts(stored_unit(deq_q), stored_unit(deq_r), n_splits, rows_per_split)


def bank_nn(deq_q, deq_r):
    return FR.bank_nn(stored_unit(deq_q), stored_unit(deq_r))


def fewshot_grid(deq_q_levels, deq_r_levels, batch, g):
    """The level-summed 1 - max cosine grid [batch, 1, g, g] (fewshot_ref.fewshot_grid on stored rows)."""
    return FR.fewshot_grid([stored_unit(q) for q in deq_q_levels], [stored_unit(r) for r in deq_r_levels], batch, g)
