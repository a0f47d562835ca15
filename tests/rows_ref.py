"""Float64 restatements of the forward row kernels (aa-clip_amd/csrc/rows.hip), written from the
formulas: plain numpy, no GPU and no aaclip import. The GPU tests (tests/test_rows_gpu.py) compare
the kernels with these; tests/test_rows_host.py pins them to torch's float64 operators, to the
float32 numpy oracle and to the golden LayerNorm vectors, and checks that the error bounds below
leave a float32 implementation a factor of two.

  layer_norm(x, w, b)            F.layer_norm over the last dim: biased variance, eps 1e-5
  blend(x, u, aw)                the adapter blend aw (u |x| / |u|) + (1 - aw) x (adapter.py:94-99)
  embed_rows(x, cls, pos, n_tok) token assembly: row t == 0 of an image is cls + pos[0], else x + pos[t]
  tap_rows(rows, n_tok)          (source rows, tap rows) of the level tap: every non-CLS row, packed
  eot_index(tokens)              the EOT position: argmax of the ids, FIRST occurrence on a tie
  anchor_reduce(emb)             normalize(mean_s normalize(emb_s)) (forward_utils.py:155-159)
  l2_normalize(x)                x / max(|x|, 1e-12)
  ln_tol / blend_tol / l2_tol    per-element error bounds of a float32 implementation
  ln_inputs(width, seed)         the LayerNorm input families the tests share
  blend_inputs(rows, width)      residual / adapter rows whose norm ratio spans 1e-3 .. 1e3
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24      # unit roundoff of float32
LN_EPS = 1e-5       # nn.LayerNorm default
L2_EPS = 1e-12      # F.normalize default
ANCHOR_ATOL = 5e-7  # anchor_reduce, absolute (unit-norm output of at most 1024 elements)


def f64(a) -> np.ndarray:
    """numpy float64 of a numpy array or a (CPU or device) torch tensor of any float dtype."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().double().numpy()
    return np.asarray(a, dtype=np.float64)


def _rstd(x):
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)  # biased
    return mean, 1.0 / np.sqrt(var + LN_EPS)


def layer_norm(x, w, b) -> np.ndarray:
    x, w, b = f64(x), f64(w), f64(b)
    mean, rstd = _rstd(x)
    return (x - mean) * rstd * w + b


def ln_tol(x, w, y_ref) -> np.ndarray:
    """|y - y_ref| allowed per element: 8 u (1 + A_row) max|w| + 2 u |y_ref|, A_row = max_j |x_j| rstd.
    x - mean carries an absolute error of about u max|x| (the rounding of the mean and of the
    difference), which rstd and w then scale; the last term is the rounding of the two final
    operations. A one-pass variance, an unbiased variance or another eps is off by orders of
    magnitude more (tests/test_rows_host.py)."""
    x, w, y_ref = f64(x), f64(w), f64(y_ref)
    _, rstd = _rstd(x)
    a_row = np.abs(x).max(-1, keepdims=True) * rstd
    return 8 * U * (1 + a_row) * np.abs(w).max() + 2 * U * np.abs(y_ref)


def _blend_terms(x, u, aw):
    x, u = f64(x), f64(u)
    aw = float(np.float32(aw))  # the value the C ABI receives
    xn = np.sqrt((x * x).sum(-1, keepdims=True))
    un = np.sqrt((u * u).sum(-1, keepdims=True))
    return aw * (u * xn / un), (1.0 - aw) * x


def blend(x, u, aw) -> np.ndarray:
    a, b = _blend_terms(x, u, aw)
    return a + b


def blend_tol(x, u, aw) -> np.ndarray:
    """8 u (|aw u_j |x| / |u|| + |(1 - aw) x_j|): a few roundings per term (two norms, a product,
    a quotient, the scaling, the sum)."""
    a, b = _blend_terms(x, u, aw)
    return 8 * U * (np.abs(a) + np.abs(b))


def embed_rows(x, cls, pos, n_tok: int) -> np.ndarray:
    """x [B * n_tok, D] (its CLS rows are never read), cls [D], pos [n_tok, D]."""
    x, cls, pos = f64(x), f64(cls).reshape(-1), f64(pos)
    t = np.arange(x.shape[0]) % n_tok
    out = x + pos[t]
    out[t == 0] = cls + pos[0]
    return out


def tap_rows(rows: int, n_tok: int):
    """(src, dst): token row src[i] (never a CLS row) lands in tap row dst[i]; the tap holds
    rows / n_tok * (n_tok - 1) rows, image-major."""
    r = np.arange(rows)
    t = r % n_tok
    src = r[t >= 1]
    dst = (src // n_tok) * (n_tok - 1) + (src % n_tok - 1)
    return src, dst


def eot_index(tokens) -> np.ndarray:
    """numpy.argmax returns the first occurrence of the maximum ("In case of multiple occurrences of
    the maximum values, the indices corresponding to the first occurrence are returned")."""
    tokens = tokens.detach().cpu().numpy() if hasattr(tokens, "detach") else np.asarray(tokens)
    return np.argmax(tokens, axis=-1)


def anchor_reduce(emb) -> np.ndarray:
    e = f64(emb)
    e = e / np.sqrt((e * e).sum(-1, keepdims=True))
    m = e.mean(0)
    return m / np.sqrt((m * m).sum())


def l2_normalize(x) -> np.ndarray:
    x = f64(x)
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), L2_EPS)


def l2_tol(y_ref) -> np.ndarray:
    return 8 * U * np.abs(f64(y_ref)) + 1e-12


# ---------------------------------------------------------------------------- shared inputs
LN_FAMILIES = ("normal", "mean100", "outlier", "small", "constant", "zero")
LN_FAMILY_ROWS = {"normal": slice(0, 3), "mean100": slice(3, 6), "outlier": slice(6, 9), "small": slice(9, 12),
                  "constant": slice(12, 14), "zero": slice(14, 15)}


def ln_inputs(width: int, seed: int = 0):
    """(x [15, width], w, b) float32: three rows each of standard normal, mean 100 / std 0.1,
    standard normal with one channel at 300 and scale 1e-4; two constant rows; one zero row.
    w = 1 + 0.1 randn, b = 0.1 randn. CLIP's residual stream looks like the second and third."""
    rng = np.random.default_rng(1000 * seed + width)
    x = rng.standard_normal((15, width))
    x[3:6] = 100.0 + 0.1 * x[3:6]
    x[6, 5] = x[7, width // 2 + 1] = x[8, width - 3] = 300.0  # one outlier channel per row, a different lane each
    x[9:12] *= 1e-4
    x[12], x[13] = 3.7, -0.01
    x[14] = 0.0
    w = 1 + 0.1 * rng.standard_normal(width)
    b = 0.1 * rng.standard_normal(width)
    return x.astype(np.float32), w.astype(np.float32), b.astype(np.float32)


def blend_inputs(rows: int, width: int, seed: int = 0):
    """(x, u) float32 [rows, width]: |x| / |u| runs from 1e-3 (first row) to 1e3 (last row)."""
    rng = np.random.default_rng(7000 + 10 * seed + width)
    x = rng.standard_normal((rows, width)) * np.logspace(-1.5, 1.5, rows)[:, None]
    u = rng.standard_normal((rows, width)) * np.logspace(1.5, -1.5, rows)[:, None]
    return x.astype(np.float32), u.astype(np.float32)
