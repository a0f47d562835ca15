"""Float64 restatement of aaclip_gemm / aaclip_gemm_scores (aa-clip_amd/csrc/gemm.hip) and the
per-element error bound the GPU tests hold the kernels to: plain numpy, no torch, no device code.
tests/test_gemm_host.py pins the reference to torch's float64 operators and checks the bound
against a float32 numpy restatement of the kernels' arithmetic; tests/test_gemm_edges_gpu.py
compares the kernels with it.

  gemm_ref(a, w, bias=, act=, residual=, row_remap=)  (float64 epilogue(A . W^T), destination rows)
  gemm_bound(a, w, ..., in16=, out=)                  per-element bound on |device - gemm_ref|
  scores_ref(v, T, t_period)                          {sum v^2, sum v t0, sum v t1, 0} per 32 columns
  scores_bound(v, ev, T, t_period)                    its bound from the bound ev on v
  gemm32 / epilogue32 / gelu_fast32 / qgelu_fast32    the float32 restatement (host checks only)
  round16(x, kind)                                    round-to-nearest-even to bf16 / fp16, as float64

The epilogue order is include/aaclip.h's: bias, erf GELU or QuickGELU, LeakyReLU(0.01), residual.
Operands arrive already rounded to their storage type (as float32 / float64 arrays holding those
values), so the reference and the kernel start from the same numbers.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24           # unit roundoff of float32
ULP = 2.0 ** -23         # one float32 ulp, relative
GELU_FAST_ABS = 2.6e-5   # common.h: |gelu_fast - erf GELU| (checked in tests/test_gemm_host.py)
QGELU_FAST_ULP = 2       # common.h: qgelu_fast2 against the exact form, in ulp of the argument
F32_ACT_ULP = 4          # erff / expf forms of the fp32 kernel: "a few ulp" of the pre-activation
# Lipschitz constants, from the functions:
#   GELU'(x) = Phi(x) + x phi(x); GELU''(x) = phi(x) (2 - x^2) = 0 at x = sqrt(2), where
#   GELU' = Phi(sqrt 2) + sqrt(2) phi(sqrt 2) = 0.921350 + 0.207554 = 1.128904
#   QuickGELU(x) = SiLU(c x) / c, so its slope is SiLU's: s (1 + t (1 - s)), s = sigmoid(t),
#   largest at t = 2.3994 where it is 1.099839
#   LeakyReLU(0.01): 1
L_GELU = 1.12891
L_QGELU = 1.09984
ACTS = ("none", "gelu", "qgelu", "leaky", "gelu+leaky", "qgelu+leaky")
_erf = np.vectorize(math.erf, otypes=[np.float64])


def f64(a) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().double().numpy()
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------- the reference
def remap_rows(M: int, row_remap):
    """Destination row of every source row: m itself, or under (row_group, row_group_out,
    row_offset) the row (m // row_group) * row_group_out + row_offset + m % row_group."""
    m = np.arange(M)
    if not row_remap or not row_remap[0]:
        return m
    g, go, off = row_remap
    return (m // g) * go + off + m % g


def act64(v, act):
    if act not in ACTS:
        raise ValueError(act)
    if "qgelu" in act:
        v = v / (1.0 + np.exp(-1.702 * v))
    elif "gelu" in act:
        v = 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))
    if "leaky" in act:
        v = np.where(v >= 0, v, 0.01 * v)
    return v


def gemm_ref(a, w, *, bias=None, act="none", residual=None, row_remap=None):
    """(out [M, N] float64, dst [M]): out[m] = act(a[m] . w^T + bias) + residual[dst[m]] is the value
    of output row dst[m]. residual is indexed by DESTINATION row (it has at least dst.max() + 1 rows),
    as the kernel reads it."""
    a, w = f64(a), f64(w)
    dst = remap_rows(a.shape[0], row_remap)
    v = a @ w.T
    if bias is not None:
        v = v + f64(bias)[None, :]
    v = act64(v, act)
    if residual is not None:
        v = v + f64(residual)[dst]
    return v, dst


# ---------------------------------------------------------------------------- 16-bit formats
def half_ulp(x, kind: str) -> np.ndarray:
    """Half the spacing of the 16-bit format at |x|: bf16 has 8 significant bits, fp16 11 with a
    subnormal spacing of 2^-24 below 2^-14."""
    bits, emin = {"bf16": (8, -126), "f16": (11, -14)}[kind]
    ax = np.abs(f64(x))
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** emin)))
    return 2.0 ** (e - bits)


def round16(x, kind: str) -> np.ndarray:
    """Round-to-nearest-even of float64 values to bf16 / fp16 (finite, in range), as float64."""
    x = f64(x)
    if kind == "f16":
        return x.astype(np.float16).astype(np.float64)
    q = 2.0 * half_ulp(x, kind)
    return np.rint(x / q) * q  # rint rounds half to even; x / q is exact (q a power of two)


# ---------------------------------------------------------------------------- the bound
def gemm_bound(a, w, *, bias=None, act="none", residual=None, row_remap=None, in16=True, out="f32"):
    """Per-element bound on |device - gemm_ref| for out in {"f32", "bf16", "f16"} (the 16-bit aux
    copy is bounded as a 16-bit C). u = 2^-24.

    Accumulation. 16-bit operands: every product a_k w_k has at most 22 significant bits, so it is
    exact in fp32, and each output is one fp32 accumulator over the K terms in some order (MFMA
    slices of 32, ascending). Any order of K - 1 fp32 additions obeys
    |fl(sum) - sum| <= gamma_{K-1} sum_k |a_k w_k| (Higham, Accuracy and Stability, 4.2), and the
    bias addition is one more rounding of a sum that includes |bias|: with
    S = sum_k |a_k| |w_k| + |bias| the pre-activation error is at most gamma_K S <= (K + 1) u S
    (the + 1 covers the second-order part of gamma_K = K u / (1 - K u) for every K below 2^11):
    c = 1. The fp32 kernel rounds each product too (or fuses it: an FMA chain), one more rounding
    per term: gamma_{K+1} S <= (K + 2) u S.

    Activation. f(v + e) differs from f(v) by at most L |e|, L the Lipschitz constant (L_GELU,
    L_QGELU, 1 for LeakyReLU, derived above from the functions). To that the form's own error:
    gelu_fast 2.6e-5 absolute against erf GELU and qgelu_fast2 2 ulp (common.h) in the 16-bit
    kernels, the ulp taken at the pre-activation |v| >= |y|: for v < 0 the rounding of the
    exponent's argument is amplified by |1.702 log2(e) v|, so in ulp of the RESULT the form is off
    by 4.8 at v = -6 and 8.4 at v = -12, while in ulp of v it stays at 1.2 everywhere (and for v >=
    0 the two agree; tests/test_gemm_host.py measures both). In the fp32 kernel erff / expf and the
    three products around them, 4 ulp of |v| (of the pre-activation, not of the result: for v < 0
    the sum 1 + erf cancels, and what is left is erf's own ulp times |v| / 2). LeakyReLU's product
    0.01f * v is one rounding, and 0.01f is 0.01 to 2.2e-8 relative: 2 u |y| together.

    Residual. One fp32 rounding of the sum: u |y + r|.

    16-bit C / aux. Round-to-nearest of a value within E of the reference is within
    E + half_ulp(|ref| + E) of it.
    """
    a, w = f64(a), f64(w)
    K = a.shape[1]
    S = np.abs(a) @ np.abs(w).T
    pre = a @ w.T
    if bias is not None:
        S = S + np.abs(f64(bias))[None, :]
        pre = pre + f64(bias)[None, :]
    E = ((K + 1) if in16 else (K + 2)) * U * S
    y = pre
    if "gelu" in act:
        quick = "qgelu" in act
        y = act64(pre, "qgelu" if quick else "gelu")
        E = (L_QGELU if quick else L_GELU) * E
        if in16:
            E = E + (QGELU_FAST_ULP * ULP * np.abs(pre) if quick else GELU_FAST_ABS)
        else:
            E = E + F32_ACT_ULP * ULP * np.abs(pre)
    if "leaky" in act:
        y = np.where(y >= 0, y, 0.01 * y)
        E = E + 2 * U * np.abs(y)
    if residual is not None:
        y = y + f64(residual)[remap_rows(a.shape[0], row_remap)]
        E = E + U * (np.abs(y) + E)
    if out != "f32":
        E = E + half_ulp(np.abs(y) + E, out)
    return E


def bound_terms(a, w, *, bias=None, act="none", residual=None, row_remap=None, in16=True, out="f32"):
    """The bound split by source, for reports: dict of per-element arrays that sum to gemm_bound
    (accumulation carried through the activation's Lipschitz constant, activation form, residual
    rounding, 16-bit rounding)."""
    kw = dict(bias=bias, row_remap=row_remap, in16=in16)
    acc = gemm_bound(a, w, act="none", out="f32", **kw)
    if "qgelu" in act:
        acc = L_QGELU * acc
    elif "gelu" in act:
        acc = L_GELU * acc
    after_act = gemm_bound(a, w, act=act, out="f32", **kw)
    after_res = gemm_bound(a, w, act=act, residual=residual, out="f32", **kw)
    total = gemm_bound(a, w, act=act, residual=residual, out=out, **kw)
    return {"accumulation": acc, "activation": after_act - acc, "residual": after_res - after_act,
            "rounding16": total - after_res}


# ---------------------------------------------------------------------------- score partials
def _anchors(T, N, t_period):
    T = f64(T)
    c = np.arange(N) % t_period
    return T[c, 0], T[c, 1]


def scores_ref(v, T, t_period: int) -> np.ndarray:
    """v [M, N] float64 (gemm_ref's value) -> part [M, N / 32, 4] =
    {sum v^2, sum v t0, sum v t1, 0} over columns 32 g .. 32 g + 31, t = T[c % t_period]."""
    v = f64(v)
    M, N = v.shape
    t0, t1 = _anchors(T, N, t_period)
    g = lambda x: x.reshape(M, N // 32, 32).sum(-1)
    return np.stack([g(v * v), g(v * t0), g(v * t1), np.zeros((M, N // 32))], axis=-1)


def scores_bound(v, ev, T, t_period: int) -> np.ndarray:
    """Bound on |device - scores_ref| from the per-element bound ev on v (gemm_bound, fp32 out).
    The device value v' = v + d, |d| <= ev, enters sums of 32 terms accumulated in fp32 (8 FMAs in a
    lane, then two levels of cross-lane additions: any order of 32 terms obeys gamma_32, and an FMA
    rounds once per term): |fl(sum x'_i) - sum x_i| <= sum |x'_i - x_i| + 33 u sum |x'_i|. For the
    squares |x' - x| <= 2 |v| ev + ev^2 and |x'| <= (|v| + ev)^2; for the anchor dots
    |x' - x| <= |t| ev and |x'| <= |t| (|v| + ev). The fourth lane is exactly 0."""
    v, ev = f64(v), f64(ev)
    M, N = v.shape
    t0, t1 = _anchors(T, N, t_period)
    g = lambda x: x.reshape(M, N // 32, 32).sum(-1)
    av = np.abs(v) + ev
    sq = g(2 * np.abs(v) * ev + ev * ev) + 33 * U * g(av * av)
    d0 = g(np.abs(t0) * ev) + 33 * U * g(np.abs(t0) * av)
    d1 = g(np.abs(t1) * ev) + 33 * U * g(np.abs(t1) * av)
    return np.stack([sq, d0, d1, np.zeros((M, N // 32))], axis=-1)


# ---------------------------------------------------------------------------- float32 restatement
_f = np.float32


def gelu_fast32(v):
    """common.h gelu_fast written out in float32 numpy: the clamp to [-8, 8], s = vc^2,
    w = vc (s (s c2 + c1) + c0) with the device's two FMAs as float64 products rounded once,
    y = v / (1 + 2^w). numpy's exp2 and division are correctly rounded where v_exp_f32 / v_rcp_f32
    are good to 1 ulp."""
    v = np.asarray(v, dtype=_f)
    vc = np.clip(v, _f(-8.0), _f(8.0))
    s = vc * vc
    fma = lambda x, y, z: (x.astype(np.float64) * np.float64(y) + np.float64(z)).astype(_f)
    inner = fma(s, _f(0.0010142630), _f(-0.10677572))
    poly = (s.astype(np.float64) * inner.astype(np.float64) + np.float64(_f(-2.3011212))).astype(_f)
    w = vc * poly
    return v * (_f(1.0) / (_f(1.0) + np.exp2(w)))


def qgelu_fast32(v):
    """common.h qgelu_fast2 in float32 numpy: v / (1 + 2^clamp(v c, -64, 64)), c = -1.702f log2(e)."""
    v = np.asarray(v, dtype=_f)
    c = _f(np.float64(_f(-1.702)) * 1.44269504088896340736)
    w = np.clip(v * c, _f(-64.0), _f(64.0))
    return v * (_f(1.0) / (_f(1.0) + np.exp2(w)))


def gemm32(a, w, *, in16=True) -> np.ndarray:
    """A . W^T with one float32 accumulator per output. 16-bit operands: slices of 32 k ascending
    (one MFMA each), the slice's 32 exact products summed in float32 in k order from zero, then
    added to the accumulator. fp32 operands: one FMA chain over k ascending (v_mfma_f32_16x16x4)."""
    a32, w32 = np.asarray(a, dtype=_f), np.asarray(w, dtype=_f)
    M, K = a32.shape
    acc = np.zeros((M, w32.shape[0]), dtype=_f)
    if in16:
        for k0 in range(0, K, 32):
            part = np.zeros_like(acc)
            for k in range(k0, k0 + 32):
                part = part + a32[:, k, None] * w32[None, :, k]
            acc = acc + part
        return acc
    a64, w64 = a32.astype(np.float64), w32.astype(np.float64)
    for k in range(K):
        acc = (acc.astype(np.float64) + a64[:, k, None] * w64[None, :, k]).astype(_f)
    return acc


def epilogue32(acc, *, bias=None, act="none", residual=None, row_remap=None, in16=True) -> np.ndarray:
    """The kernels' epilogue in float32 numpy, in the header's order. 16-bit kernels: gelu_fast /
    qgelu_fast2; fp32 kernel: 0.5 v (1 + erf(v / sqrt 2)) and v / (1 + exp(-1.702 v)) in float32."""
    v = np.asarray(acc, dtype=_f)
    if bias is not None:
        v = v + np.asarray(bias, dtype=_f)[None, :]
    if "qgelu" in act:
        v = qgelu_fast32(v) if in16 else v * (_f(1.0) / (_f(1.0) + np.exp(_f(-1.702) * v)))
    elif "gelu" in act:
        if in16:
            v = gelu_fast32(v)
        else:
            e = _erf((v * _f(0.70710678118654752440)).astype(np.float64)).astype(_f)
            v = _f(0.5) * v * (_f(1.0) + e)
    if "leaky" in act:
        v = np.where(v >= 0, v, _f(0.01) * v)
    if residual is not None:
        v = v + np.asarray(residual, dtype=_f)[remap_rows(v.shape[0], row_remap)]
    assert v.dtype == _f
    return v


def scores32(v, T, t_period: int) -> np.ndarray:
    """The partials of float32 v summed in float32, column order."""
    v = np.asarray(v, dtype=_f)
    M, N = v.shape
    t0, t1 = (x.astype(_f) for x in _anchors(T, N, t_period))
    out = np.zeros((M, N // 32, 4), dtype=_f)
    for i, x in enumerate((v * v, v * t0, v * t1)):
        x = x.reshape(M, N // 32, 32)
        s = np.zeros((M, N // 32), dtype=_f)
        for c in range(32):
            s = s + x[:, :, c]
        out[:, :, i] = s
    return out


# ---------------------------------------------------------------------------- shared inputs
EPILOGUES = {  # name -> (bias, act, residual, aux, remap)
    "none": (False, "none", False, False, False),
    "bias": (True, "none", False, False, False),
    "bias+gelu": (True, "gelu", False, False, False),
    "bias+qgelu": (True, "qgelu", False, False, False),
    "leaky": (False, "leaky", False, False, False),
    "bias+resid": (True, "none", True, False, False),
    "bias+resid+aux": (True, "none", True, True, False),
    "leaky+resid": (False, "leaky", True, False, False),
    "bias+gelu+resid+aux": (True, "gelu", True, True, False),
    "bias+aux": (True, "none", False, True, False),
    "remap": (False, "none", False, False, True),
    "remap+resid+aux": (False, "none", True, True, True),
}
REMAP = (5, 7, 2)  # row_group, row_group_out, row_offset: a group that divides no tile


def rows_out(M: int, row_remap) -> int:
    return int(remap_rows(M, row_remap).max()) + 1


def gemm_inputs(M: int, N: int, K: int, kind: str, seed: int = 0, row_remap=None):
    """Operands already rounded to `kind` ("bf16", "f16" or "f32") as float32 arrays: a [M, K]
    standard normal, w [N, K] normal / sqrt(K) (pre-activations of unit scale, where the GELUs
    bend), bias [N] 0.5 normal, residual [rows_out, N] normal, anchors T [t, 2] for the scores."""
    rng = np.random.default_rng(100003 * seed + 1009 * M + 17 * N + K)
    rnd = (lambda x: x.astype(np.float32)) if kind == "f32" else (lambda x: round16(x, kind).astype(np.float32))
    a = rnd(rng.standard_normal((M, K)))
    w = rnd(rng.standard_normal((N, K)) / math.sqrt(K))
    bias = (0.5 * rng.standard_normal(N)).astype(np.float32)
    resid = rng.standard_normal((rows_out(M, row_remap), N)).astype(np.float32)
    return a, w, bias, resid


def anchors(t_period: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(77 + seed).standard_normal((t_period, 2)).astype(np.float32) / 8
