"""Float64 restatements of the backward row kernels (aa-clip_amd/csrc/text_bwd.hip, visual_bwd.hip
and layer_norm_bwd of rowmath.h), written from the formulas in the kernels' comments: plain numpy, no
GPU and no aaclip import. The GPU tests (tests/test_rows_bwd_gpu.py) compare the kernels with these
element by element; tests/test_rows_bwd_host.py pins them to torch's float64 autograd, checks that
two float32 CPU implementations use at most half of each bound, and that a list of wrong formulas
leaves it.

  layer_norm_bwd(dy, x, w)                  rowmath.h: "g = dy w, xh = (x - mean) rstd,
                                            dx = rstd (g - mean(g) - xh mean(g xh))"
  tap_ln_bwd(dtap, x, w, g, batch, n_tok)   visual_bwd.hip: "Token row (b, t >= 1) of g +=
                                            LN_bwd(dtap[b, t - 1]; x[b, t], w)", CLS rows untouched
  eot_ln_bwd(dy, x, tokens, w)              text_bwd.hip: "row (s, t) of g is LN_bwd(dy[s]; x[s, t]) at
                                            t = the first argmax of tokens[s], zero elsewhere"
  l2_normalize_bwd(dy, x, group, scale)     visual_bwd.hip: "gy = scale * dy[row / group];
                                            |x| > 1e-12: dx = (gy - y (y . gy)) / |x|;
                                            |x| <= 1e-12: dx = gy / 1e-12"
  blend_bwd(dy, x, u, aw) -> (dx, du)       text_bwd.hip: "a = sum dy u; dx = (1 - w) dy +
                                            w (a / |u|) x / |x|; du = w (|x| / |u|) (dy - u a / |u|^2)"
  anchor_reduce_bwd(emb, g)                 text_bwd.hip: "dm = (g - t (t . g)) / |m|;
                                            de_s = (dm / n - eh_s (eh_s . dm / n)) / |e_s|"
  linear_wgrad(dy, x)                       text_bwd.hip: "dW[n, k] = sum_m dY[m, n] X[m, k]"
  *_tol(...)                                per-element error bounds of a float32 implementation

The bounds are first-order running error analyses of the formula as written, in units of the unit
roundoff u (an argument, so the float64 check uses the same functions with u = 2^-53). Two
conventions are shared by all of them:

  * a sum over a row costs at most SUM_OPS = 24 roundings: one wave owns a row, a lane adds its
    4 VEC <= 16 elements in order and the butterfly adds 6 more levels (22), and the scaling by 1 / D
    or the product under the sum adds the rest. A sum of terms t_j is therefore off by at most
    SUM_OPS u sum |t_j|. A longer serial chain (a CPU vector loop) has a larger worst case but its
    roundings do not line up; the host test checks what two such implementations really use.
  * the LayerNorm statistics follow rows_ref.ln_tol: x_j - mean is taken to carry an absolute error
    of 8 u max|x|, so with A = max|x| rstd the normalised xh_j is off by 8 u A + |xh_j| (dr + u),
    where dr = (SUM_OPS / 2 + 2) u + 8 u A bounds the relative error of rstd (the variance is a sum
    of squares of those differences: 2 * 8 u max|x| mean|x - mean| / var <= 16 u A, halved by the
    square root, plus the sum's own SUM_OPS u, halved, and the division and square root).
"""
from __future__ import annotations

import numpy as np

import rows_ref as RR

U = RR.U
U64 = 2.0 ** -53    # unit roundoff of float64
SUM_OPS = 24        # roundings charged to one sum over a row (see the module docstring)
WGRAD_ROWS = 64     # AACLIP_WGRAD_ROWS: rows per partial sum of linear_wgrad
f64 = RR.f64


def _abs(a):
    return np.abs(a)


# ---------------------------------------------------------------------------- LayerNorm backward
def _ln_parts(dy, x, w):
    dy, x, w = f64(dy), f64(x), f64(w)
    mean, rstd = RR._rstd(x)
    xh = (x - mean) * rstd
    g = dy * w
    return g, xh, rstd, g.mean(-1, keepdims=True), (g * xh).mean(-1, keepdims=True)


def layer_norm_bwd(dy, x, w) -> np.ndarray:
    """dx of y = LN(x; w, b) for the upstream dy: rstd (g - mean(g) - xh mean(g xh)), g = dy w."""
    g, xh, rstd, s1, s2 = _ln_parts(dy, x, w)
    return rstd * (g - s1 - xh * s2)


def ln_bwd_tol(dy, x, w, u: float = U) -> np.ndarray:
    """Per element, with kx_j = 8 u A + |xh_j| (dr + u) the error of xh_j (module docstring):
      g_j = dy_j w_j                 u |g_j|
      s1 = mean(g)                   ds1 = (SUM_OPS + 1) u mean|g|
      s2 = mean(g xh)                ds2 = (SUM_OPS + 2) u mean|g xh| + mean(|g| kx)
      t_j = g_j - s1 - xh_j s2       dt_j = u |g_j| + ds1 + kx_j |s2| + |xh_j| ds2 + u |xh_j s2|
                                            + 2 u (|g_j| + |s1| + |xh_j s2|)   (the two subtractions)
      dx_j = rstd t_j                rstd dt_j + |dx_j| (dr + u)
    The cancellation in t_j is what makes this a per-element absolute bound: none of the terms
    shrinks with |dx_j|."""
    g, xh, rstd, s1, s2 = _ln_parts(dy, x, w)
    a_row = _abs(f64(x)).max(-1, keepdims=True) * rstd
    dr = (SUM_OPS / 2 + 2) * u + 8 * u * a_row
    kx = 8 * u * a_row + _abs(xh) * (dr + u)
    ds1 = (SUM_OPS + 1) * u * _abs(g).mean(-1, keepdims=True)
    ds2 = (SUM_OPS + 2) * u * _abs(g * xh).mean(-1, keepdims=True) + (_abs(g) * kx).mean(-1, keepdims=True)
    dt = (u * _abs(g) + ds1 + kx * _abs(s2) + _abs(xh) * ds2 + u * _abs(xh * s2)
          + 2 * u * (_abs(g) + _abs(s1) + _abs(xh * s2)))
    return rstd * dt + _abs(rstd * (g - s1 - xh * s2)) * (dr + u)


def tap_ln_bwd(dtap, x, w, g, batch: int, n_tok: int) -> np.ndarray:
    """g with LN_bwd(dtap[b, t - 1]; x[b, t], w) added to every token row t >= 1; the CLS rows are g's."""
    out = f64(g).copy()
    assert out.shape[0] == batch * n_tok
    src, dst = RR.tap_rows(batch * n_tok, n_tok)
    out[src] += layer_norm_bwd(f64(dtap)[dst], f64(x)[src], w)
    return out


def tap_ln_bwd_tol(dtap, x, w, g, batch: int, n_tok: int, u: float = U) -> np.ndarray:
    """ln_bwd_tol of the row's LayerNorm backward plus u |result| for the accumulation; exactly 0 on
    the CLS rows, which the kernel must not touch."""
    ref = tap_ln_bwd(dtap, x, w, g, batch, n_tok)
    src, dst = RR.tap_rows(batch * n_tok, n_tok)
    tol = np.zeros_like(ref)
    tol[src] = ln_bwd_tol(f64(dtap)[dst], f64(x)[src], w, u) + u * _abs(ref[src])
    return tol


def _eot_rows(tokens):
    idx = RR.eot_index(tokens)
    return np.arange(idx.shape[0]) * np.asarray(tokens.shape)[-1] + idx


def eot_ln_bwd(dy, x, tokens, w) -> np.ndarray:
    """[n ctx, width]: LN_bwd(dy[s]; x[s, t]) in row (s, t = eot_index(tokens[s])), zero elsewhere."""
    x = f64(x)
    rows = _eot_rows(tokens)
    out = np.zeros_like(x)
    out[rows] = layer_norm_bwd(dy, x[rows], w)
    return out


def eot_ln_bwd_tol(dy, x, tokens, w, u: float = U) -> np.ndarray:
    """ln_bwd_tol in the EOT rows; exactly 0 elsewhere (those rows are written as zeros)."""
    x = f64(x)
    rows = _eot_rows(tokens)
    tol = np.zeros_like(x)
    tol[rows] = ln_bwd_tol(dy, x[rows], w, u)
    return tol


# ---------------------------------------------------------------------------- l2_normalize backward
def _l2_parts(dy, x, group: int, scale: float):
    dy, x = f64(dy), f64(x)
    scale = float(np.float32(scale))  # the value the C ABI receives
    r = np.arange(x.shape[0])
    gy = scale * dy[r // group if group > 0 else r]
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    return gy, x, n


def l2_normalize_bwd(dy, x, group: int = 0, scale: float = 1.0) -> np.ndarray:
    """dx of y = x / max(|x|, 1e-12) for gy = scale dy[r // group] (group 0: dy[r]):
    |x| > 1e-12: (gy - y (y . gy)) / |x|; |x| <= 1e-12: gy / 1e-12, the clamp passes no gradient to
    the norm."""
    gy, x, n = _l2_parts(dy, x, group, scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = x / n
        reg = (gy - y * (y * gy).sum(-1, keepdims=True)) / n
    return np.where(n > RR.L2_EPS, reg, gy / RR.L2_EPS)


def l2_bwd_tol(dy, x, group: int = 0, scale: float = 1.0, u: float = U) -> np.ndarray:
    """Regular branch, rn = (SUM_OPS / 2 + 2) u the relative error of 1 / |x| (a sum of squares, a
    square root, a division) and ry = rn + u that of y_j:
      gy_j = scale dy_j              u |gy_j|
      a = y . gy                     da = (SUM_OPS + 1 + ry / u + 1) u sum|y gy|
      t_j = gy_j - y_j a             dt_j = u |gy_j| + |y_j| da + |y_j a| (ry + u) + u (|gy_j| + |y_j a|)
      dx_j = t_j / |x|               dt_j / |x| + |dx_j| (rn + u)
    Clamp branch: gy_j / 1e-12 is two products by constants, neither of them a float32 (scale = 1 / 5 and
    1e12 are off by up to u and 0.07 u; a division by 1e-12 by 0.3 u): 8 u |dx_j|, the allowance
    rows_ref gives an elementwise result of a few roundings."""
    gy, x, n = _l2_parts(dy, x, group, scale)
    ref = l2_normalize_bwd(dy, x, group, scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = x / n
        a = (y * gy).sum(-1, keepdims=True)
        rn = (SUM_OPS / 2 + 2) * u
        ry = rn + u
        da = ((SUM_OPS + 2) * u + ry) * _abs(y * gy).sum(-1, keepdims=True)
        dt = u * _abs(gy) + _abs(y) * da + _abs(y * a) * (ry + u) + u * (_abs(gy) + _abs(y * a))
        reg = dt / n + _abs(ref) * (rn + u)
    return np.where(n > RR.L2_EPS, reg, 8 * u * _abs(ref))


# ---------------------------------------------------------------------------- adapter blend backward
def _blend_parts(dy, x, u_, aw):
    dy, x, u_ = f64(dy), f64(x), f64(u_)
    aw = float(np.float32(aw))  # the value the C ABI receives
    xn = np.sqrt((x * x).sum(-1, keepdims=True))
    uq = (u_ * u_).sum(-1, keepdims=True)
    a = (dy * u_).sum(-1, keepdims=True)
    return dy, x, u_, aw, xn, uq, np.sqrt(uq), a


def blend_bwd(dy, x, u_, aw):
    """(dx, du) of y = aw u |x| / |u| + (1 - aw) x: dx = (1 - aw) dy + aw (a / |u|) x / |x| (the direct
    path and the path through |x|), du = aw (|x| / |u|) (dy - u a / |u|^2), a = sum dy u."""
    dy, x, u_, aw, xn, uq, un, a = _blend_parts(dy, x, u_, aw)
    return (1.0 - aw) * dy + aw * (a / un) / xn * x, aw * (xn / un) * (dy - u_ * (a / uq))


def blend_bwd_tol(dy, x, u_, aw, u: float = U):
    """(tol_dx, tol_du). rn = (SUM_OPS / 2 + 1) u is the relative error of |x| and of |u|, SUM_OPS u
    that of |u|^2, da = (SUM_OPS + 1) u sum|dy u| the error of a (which may exceed |a|):
      cx = aw (a / |u|) / |x|        dcx = aw da / (|u| |x|) + |cx| (2 rn + 3 u)
      dx_j = keep dy_j + cx x_j      8 u (|keep dy_j| + |cx x_j|) + |x_j| dcx
                                     (rows_ref.blend_tol's allowance for the few roundings of the two
                                     terms: keep = 1 - aw, the products, the sum, one FMA or none)
      au = a / |u|^2                 dau = da / |u|^2 + |au| (SUM_OPS + 1) u
      in_j = dy_j - u_j au           din_j = |u_j| dau + u |u_j au| + u |in_j|
      du_j = cu in_j, cu = aw |x| / |u|     cu din_j + |du_j| (2 rn + 3 u)
    At aw = 0 both reduce to 0 beside 8 u |dy_j|; the GPU test asks for exact bits there."""
    dy, x, u_, aw, xn, uq, un, a = _blend_parts(dy, x, u_, aw)
    dx, du = blend_bwd(dy, x, u_, aw)
    rn = (SUM_OPS / 2 + 1) * u
    da = (SUM_OPS + 1) * u * _abs(dy * u_).sum(-1, keepdims=True)
    cx = aw * (a / un) / xn
    dcx = aw * da / (un * xn) + _abs(cx) * (2 * rn + 3 * u)
    tol_dx = 8 * u * (_abs((1.0 - aw) * dy) + _abs(cx * x)) + _abs(x) * dcx
    au = a / uq
    dau = da / uq + _abs(au) * (SUM_OPS + 1) * u
    din = _abs(u_) * dau + u * _abs(u_ * au) + u * _abs(dy - u_ * au)
    tol_du = aw * (xn / un) * din + _abs(du) * (2 * rn + 3 * u)
    return tol_dx, tol_du


# ---------------------------------------------------------------------------- anchor backward
def anchor_reduce_bwd(emb, g) -> np.ndarray:
    """demb [n, dim] of t = m / |m|, m = mean_s e_s / |e_s| for the upstream g [dim]:
    dm = (g - t (t . g)) / |m|, de_s = (dm / n - eh_s (eh_s . dm / n)) / |e_s|, eh_s = e_s / |e_s|."""
    e, g = f64(emb), f64(g).reshape(-1)
    n = e.shape[0]
    en = np.sqrt((e * e).sum(-1, keepdims=True))
    eh = e / en
    m = eh.mean(0)
    mn = np.sqrt((m * m).sum())
    t = m / mn
    dmn = (g - t * (t * g).sum()) / mn / n
    return (dmn - eh * (eh * dmn).sum(-1, keepdims=True)) / en


def anchor_bwd_tol(emb, g, u: float = U) -> np.ndarray:
    """The formula's steps, each with the error it inherits and the roundings it adds. re =
    (SUM_OPS / 2 + 2) u is the relative error of 1 / |e_s|, M_j = mean_s |eh_sj|:
      m_j = mean_s eh_sj             dm_j = (n + re / u + 2) u M_j     (n terms added in index order)
      |m|^2, 1 / |m|                 rm = (sum_j 2 |m_j| dm_j + SUM_OPS u |m|^2) / (2 |m|^2) + 2 u
      m . g                          dmg = sum_j |g_j| dm_j + SUM_OPS u sum|m g|
      tg = (m . g) / |m|             dtg = dmg / |m| + |tg| (rm + u)
      t_j = m_j / |m|                dt_j = dm_j / |m| + |t_j| (rm + u)
      p_j = g_j - t_j tg             dp_j = dt_j |tg| + |t_j| dtg + 2 u (|g_j| + |t_j tg|)
      d_j = p_j / |m| / n            dd_j = dp_j / (|m| n) + |d_j| (rm + 3 u)
      c_s = eh_s . d                 dc_s = sum_j |eh_sj| dd_j + (SUM_OPS + re / u + 2) u sum_j |eh_sj d_j|
      q_sj = d_j - eh_sj c_s         dq_sj = dd_j + |eh_sj| dc_s + |eh_sj c_s| (re + 2 u) + u (|d_j| + |eh_sj c_s|)
      de_sj = q_sj / |e_s|           dq_sj / |e_s| + |de_sj| (re + u)"""
    e, g = f64(emb), f64(g).reshape(-1)
    n = e.shape[0]
    en = np.sqrt((e * e).sum(-1, keepdims=True))
    eh = e / en
    re = (SUM_OPS / 2 + 2) * u
    m = eh.mean(0)
    dm = ((n + 2) * u + re) * _abs(eh).mean(0)
    mm = (m * m).sum()
    mn = np.sqrt(mm)
    rm = ((2 * _abs(m) * dm).sum() + SUM_OPS * u * mm) / (2 * mm) + 2 * u
    dmg = (_abs(g) * dm).sum() + SUM_OPS * u * _abs(m * g).sum()
    tg = (m * g).sum() / mn
    dtg = dmg / mn + abs(tg) * (rm + u)
    t = m / mn
    dt = dm / mn + _abs(t) * (rm + u)
    dp = dt * abs(tg) + _abs(t) * dtg + 2 * u * (_abs(g) + _abs(t * tg))
    d = (g - t * tg) / mn / n
    dd = dp / (mn * n) + _abs(d) * (rm + 3 * u)
    c = (eh * d).sum(-1, keepdims=True)
    dc = (_abs(eh) * dd).sum(-1, keepdims=True) + ((SUM_OPS + 2) * u + re) * _abs(eh * d).sum(-1, keepdims=True)
    dq = dd + _abs(eh) * dc + _abs(eh * c) * (re + 2 * u) + u * (_abs(d) + _abs(eh * c))
    return dq / en + _abs((d - eh * c) / en) * (re + u)


# ---------------------------------------------------------------------------- Linear weight gradient
def linear_wgrad(dy, x) -> np.ndarray:
    """dW [N, K] = sum_m dY[m, n] X[m, k]."""
    return f64(dy).T @ f64(x)


def wgrad_tol(dy, x, u: float = U) -> np.ndarray:
    """(min(M, 64) + 1) u sum_m |dY[m, n]| |X[m, k]|: a partial sum takes at most WGRAD_ROWS = 64 rows,
    one rounding (an FMA) per row; the partials are added in float64 and the result is rounded once."""
    dy, x = f64(dy), f64(x)
    return (min(dy.shape[0], WGRAD_ROWS) + 1) * u * (_abs(dy).T @ _abs(x))


# ---------------------------------------------------------------------------- shared inputs
def ln_bwd_inputs(width: int, seed: int = 0):
    """(dy, x, w) float32 [15, width]: rows_ref.ln_inputs' x and w (their families, LN_FAMILY_ROWS) and a
    standard normal dy whose rows differ in scale by up to 4."""
    x, w, _ = RR.ln_inputs(width, seed)
    rng = np.random.default_rng(2000 * seed + width + 1)
    dy = rng.standard_normal(x.shape) * (1 + np.arange(x.shape[0]) % 4)[:, None]
    return dy.astype(np.float32), x, w


L2_FAMILIES = ("ordinary", "zero", "clamp", "tiny")
L2_FAMILY_ROWS = {"ordinary": [0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 14], "zero": [4], "clamp": [9], "tiny": [13]}


def l2_bwd_inputs(width: int, seed: int = 0):
    """(dy [15, width], dy_group [3, width], x [15, width]) float32. x: ordinary rows of norms from about
    3e-2 to 3e4, row 4 all zero, row 9 a unit row scaled to norm 1e-13 (both take the clamp branch) and
    row 13 one scaled to 1e-11 (the regular branch, 10 times above the clamp)."""
    rng = np.random.default_rng(3000 + 10 * seed + width)
    x = rng.standard_normal((15, width)) * np.logspace(-3, 3, 15)[:, None]
    unit = rng.standard_normal((2, width))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    x[4], x[9], x[13] = 0.0, 1e-13 * unit[0], 1e-11 * unit[1]
    dy = rng.standard_normal((15, width))
    dyg = rng.standard_normal((3, width))
    return dy.astype(np.float32), dyg.astype(np.float32), x.astype(np.float32)


def blend_bwd_inputs(rows: int, width: int, seed: int = 0):
    """(dy, x, u) float32: rows_ref.blend_inputs' x and u (|x| / |u| from 1e-3 to 1e3) and a standard normal dy."""
    x, u_ = RR.blend_inputs(rows, width, seed)
    dy = np.random.default_rng(7500 + 10 * seed + width).standard_normal((rows, width))
    return dy.astype(np.float32), x, u_


ANCHOR_NS, ANCHOR_DIMS = (1, 2, 5, 35, 256), (100, 520, 768, 1024)


def anchor_bwd_inputs(n: int, dim: int):
    """(emb [n, dim], dT column g [dim]) float32: correlated prompts (a shared direction plus half as
    much noise) whose norms run from 1e-2 to 1e2."""
    rng = np.random.default_rng(1000 * n + dim + 5)
    e = (rng.standard_normal(dim) + 0.5 * rng.standard_normal((n, dim))) * np.logspace(-2, 2, n)[:, None]
    return e.astype(np.float32), rng.standard_normal(dim).astype(np.float32)


WGRAD_MS, WGRAD_NKS = (1, 15, 16, 17, 63, 64, 65, 128, 129), ((64, 64), (64, 192), (192, 64))


def wgrad_inputs(M: int, N: int, K: int, exact: bool = False):
    """(dY [M, N], X [M, K]) float32: standard normal, or integers -3 .. 3 (every product and every
    partial sum is then an integer below 129 * 9 < 2^24, exact in float32 in any order)."""
    rng = np.random.default_rng(100 * M + N + 3 * K + int(exact))
    if exact:
        return (rng.integers(-3, 4, (M, N)).astype(np.float32), rng.integers(-3, 4, (M, K)).astype(np.float32))
    return rng.standard_normal((M, N)).astype(np.float32), rng.standard_normal((M, K)).astype(np.float32)
