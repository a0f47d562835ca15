"""Host-side checks of the backward row kernels' references (no GPU): every closed form of
tests/rows_bwd_ref.py equals torch's float64 autograd; two independent float32 CPU implementations
(torch's float32 autograd, and a numpy float32 restatement in the kernel's order of operations) use
at most half of each per-element bound on every input family; a list of wrong formulas, computed in
float64, leaves the bound; and the ops wrappers reject overlapping operands without a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aaclip import ops

import rows_bwd_ref as RB
import rows_ref as RR

WIDTHS = (768, 1024)
F32 = np.float32
# Both sides of the float64 comparison are float64 evaluations of the same formula in another order,
# each within the bound at u = 2^-53 of the exact value: their difference is allowed twice that.
F64_MULT = 2.0


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def _worst(got, ref, tol):
    """Worst |got - ref| / tol over the elements; an error where the bound is 0 counts as infinite."""
    err = np.abs(RR.f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / tol, 0.0)
    assert not np.isnan(ratio).any()
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------- torch autograd, either precision
def _ln_torch(dy, x, w, dt):
    xt = _t(x, dt).requires_grad_()
    F.layer_norm(xt, (x.shape[-1],), _t(w, dt), None, 1e-5).backward(_t(dy, dt))
    return xt.grad.numpy()


def _tap_torch(dtap, x, w, g, batch, n_tok, dt):
    xt = _t(x, dt).requires_grad_()
    y = F.layer_norm(xt, (x.shape[-1],), _t(w, dt), None, 1e-5)
    y.view(batch, n_tok, -1)[:, 1:].reshape(dtap.shape).backward(_t(dtap, dt))  # the level tap: every non-CLS row
    return (_t(g, dt) + xt.grad).numpy()


def _eot_torch(dy, x, tokens, w, dt):
    n, ctx = tokens.shape
    xt = _t(x, dt).requires_grad_()
    pick = xt.view(n, ctx, -1)[torch.arange(n), torch.from_numpy(tokens).long().argmax(-1)]
    assert np.array_equal(torch.from_numpy(tokens).long().argmax(-1).numpy(), RR.eot_index(tokens))
    F.layer_norm(pick, (x.shape[-1],), _t(w, dt), None, 1e-5).backward(_t(dy, dt))
    return xt.grad.numpy()


def _l2_torch(dy, x, group, scale, dt):
    xt = _t(x, dt).requires_grad_()
    y = F.normalize(xt, dim=-1)
    if group:
        y = y.view(-1, group, x.shape[-1]).sum(1) * float(F32(scale))
    y.backward(_t(dy, dt))
    return xt.grad.numpy()


def _blend_torch(dy, x, u, aw, dt):
    xt, ut = _t(x, dt).requires_grad_(), _t(u, dt).requires_grad_()
    a = float(F32(aw))
    y = a * (ut * xt.norm(dim=-1, keepdim=True) / ut.norm(dim=-1, keepdim=True)) + (1 - a) * xt
    y.backward(_t(dy, dt))
    return xt.grad.numpy(), ut.grad.numpy()


def _anchor_torch(e, g, dt):
    et = _t(e, dt).requires_grad_()
    F.normalize(F.normalize(et, dim=-1).mean(0), dim=0).backward(_t(g, dt))
    return et.grad.numpy()


def _wgrad_torch(dy, x, dt):
    w = torch.zeros(dy.shape[1], x.shape[1], dtype=dt, requires_grad=True)
    F.linear(_t(x, dt), w).backward(_t(dy, dt))
    return w.grad.numpy()


# ---------------------------------------------------------------------------- the kernels' order, in numpy float32
def _lanes(a):
    """[rows, 256 VEC] -> [rows, VEC, 64, 4]: lane l holds elements 256 c + 4 l .. + 3 (rowmath.h)."""
    a = np.asarray(a, F32)
    return a.reshape(a.shape[0], a.shape[1] // 256, 64, 4)


def _wave_sum(p):
    """wave_sum of [..., 64] lane values: the xor butterfly 32, 16, .. 1 (addition commutes, so every
    lane ends with the same tree)."""
    for o in (32, 16, 8, 4, 2, 1):
        p = p[..., :o] + p[..., o:2 * o]
    assert p.dtype == F32
    return p


def _row_dot32(a, b):
    A, B = _lanes(a), _lanes(b)
    s = np.zeros(A.shape[:1] + (64,), F32)
    for c in range(A.shape[1]):
        for j in range(4):
            s = s + A[:, c, :, j] * B[:, c, :, j]
    return _wave_sum(s)


def _ln_stats32(x):
    X = _lanes(x)
    inv_d = F32(1.0) / F32(x.shape[1])
    s = np.zeros(X.shape[:1] + (64,), F32)
    for c in range(X.shape[1]):
        s = s + ((X[:, c, :, 0] + X[:, c, :, 1]) + (X[:, c, :, 2] + X[:, c, :, 3]))
    mean = _wave_sum(s) * inv_d
    q = np.zeros_like(s)
    for c in range(X.shape[1]):
        for j in range(4):
            d = X[:, c, :, j] - mean
            q = q + d * d
    return mean, F32(1.0) / np.sqrt(_wave_sum(q) * inv_d + F32(1e-5))


def _ln_bwd32(dy, x, w):
    """layer_norm_bwd of rowmath.h without the FMA contraction a compiler may add."""
    mean, rstd = _ln_stats32(x)
    inv_d = F32(1.0) / F32(x.shape[1])
    g = np.asarray(dy, F32) * np.asarray(w, F32)
    xh = (np.asarray(x, F32) - mean) * rstd
    G, XH = _lanes(g), _lanes(xh)
    s1 = np.zeros(G.shape[:1] + (64,), F32)
    s2 = np.zeros_like(s1)
    for c in range(G.shape[1]):
        for j in range(4):
            s1 = s1 + G[:, c, :, j]
            s2 = s2 + G[:, c, :, j] * XH[:, c, :, j]
    s1, s2 = _wave_sum(s1) * inv_d, _wave_sum(s2) * inv_d
    out = rstd * (g - s1 - xh * s2)
    assert out.dtype == F32
    return out


def _l2_bwd32(dy, x, group, scale):
    x = np.asarray(x, F32)
    r = np.arange(x.shape[0])
    gy = np.asarray(dy, F32)[r // group if group else r] * F32(scale)
    n = np.sqrt(_row_dot32(x, x))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F32(1.0) / n
        y = x * inv
        a = _row_dot32(np.where(np.isfinite(y), y, F32(0)), gy)
        reg = (gy - y * a) * inv
    out = np.where(n > F32(1e-12), reg, gy * F32(1e12))
    assert out.dtype == F32
    return out


def _blend_bwd32(dy, x, u, aw):
    dy, x, u = (np.asarray(a, F32) for a in (dy, x, u))
    aw = F32(aw)
    xn = np.sqrt(_row_dot32(x, x))
    uq = _row_dot32(u, u)
    un = np.sqrt(uq)
    a = _row_dot32(dy, u)
    keep = F32(1.0) - aw
    cx, cu, au = aw * (a / un) / xn, aw * (xn / un), a / uq
    dx, du = keep * dy + cx * x, cu * (dy - u * au)
    assert dx.dtype == F32 and du.dtype == F32
    return dx, du


def _strided_sum32(a, stride):
    """Thread / lane t adds elements t, t + stride, .. of the last axis in order -> [..., stride]."""
    pad = -a.shape[-1] % stride
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (pad,), F32)], -1).reshape(a.shape[:-1] + (-1, stride))
    s = np.zeros(a.shape[:-2] + (stride,), F32)
    for c in range(a.shape[-2]):
        s = s + a[..., c, :]
    return s


def _anchor_bwd32(e, g):
    """anchor_reduce_bwd_kernel: a lane's strided sums, then the butterfly; thread j owns columns j, j + 256,
    ..; the block sums are (w0 + w1) + (w2 + w3) of the four waves."""
    e, g = np.asarray(e, F32), np.asarray(g, F32)
    n, dim = e.shape
    inv = F32(1.0) / np.sqrt(_wave_sum(_strided_sum32(e * e, 64)))  # [n, 1]
    acc = np.zeros(dim, F32)
    for s in range(n):
        acc = acc + e[s] * inv[s]
    m = acc / F32(n)

    def block_sum(v):
        w = _wave_sum(_strided_sum32(v, 256).reshape(4, 64))[:, 0]
        return (w[0] + w[1]) + (w[2] + w[3])

    inv_m = F32(1.0) / np.sqrt(block_sum(m * m))
    tg = block_sum(m * g) * inv_m
    dm = (g - m * inv_m * tg) * inv_m / F32(n)
    d = _wave_sum(_strided_sum32(e * inv * dm, 64))
    out = (dm - e * inv * d) * inv
    assert out.dtype == F32
    return out


def _wgrad32(dy, x):
    """linear_wgrad_kernel: 64-row chunks added row by row in float32, the chunks then in float64."""
    dy, x = np.asarray(dy, F32), np.asarray(x, F32)
    total = np.zeros((dy.shape[1], x.shape[1]), np.float64)
    for m0 in range(0, dy.shape[0], RB.WGRAD_ROWS):
        acc = np.zeros(total.shape, F32)
        for m in range(m0, min(m0 + RB.WGRAD_ROWS, dy.shape[0])):
            acc = acc + dy[m][:, None] * x[m][None, :]
        total += acc
    return total.astype(F32)


# ---------------------------------------------------------------------------- the cases
BLEND_FAMILY_ROWS = {"low": slice(0, 5), "mid": slice(5, 10), "high": slice(10, 15)}  # |x| / |u|: 1e-3 .. 1e3


def _tap_case(width, batch, n_tok):
    rng = np.random.default_rng(width + n_tok)
    x = RR.ln_inputs(width, seed=1)[0][:batch * n_tok]
    w = RR.ln_inputs(width, seed=1)[1]
    dtap = rng.standard_normal((batch * (n_tok - 1), width)).astype(F32)
    g = rng.standard_normal((batch * n_tok, width)).astype(F32)
    return dtap, x, w, g


def _eot_case(width, ctx=7):
    rng = np.random.default_rng(width + ctx)
    tok = rng.integers(1, 40, (3, ctx)).astype(np.int32)
    tok[0, 0] = tok[1, ctx - 1] = tok[2, 2] = tok[2, 5] = 49407  # first, last, a tie
    x = (rng.standard_normal((3 * ctx, width)) * 2 + 0.3).astype(F32)
    return rng.standard_normal((3, width)).astype(F32), x, tok, RR.ln_inputs(width)[1]


def _cases(width):
    """Every closed form on its input families: (name, {family: rows}, ref, tol(u), torch(dt), numpy32)."""
    out = []
    dy, x, w = RB.ln_bwd_inputs(width)
    out.append((f"layer_norm_bwd {width}", RR.LN_FAMILY_ROWS, RB.layer_norm_bwd(dy, x, w),
                lambda u, a=(dy, x, w): RB.ln_bwd_tol(*a, u), lambda dt, a=(dy, x, w): _ln_torch(*a, dt),
                lambda a=(dy, x, w): _ln_bwd32(*a)))
    for batch, n_tok in ((3, 5), (3, 2)):
        tc = _tap_case(width, batch, n_tok)

        def tap32(tc=tc, n_tok=n_tok):
            src, dst = RR.tap_rows(tc[1].shape[0], n_tok)
            o = tc[3].copy()
            o[src] = tc[3][src] + _ln_bwd32(tc[0][dst], tc[1][src], tc[2])
            return o
        out.append((f"tap_ln_bwd {width} n_tok {n_tok}", {"all": slice(None)}, RB.tap_ln_bwd(*tc, batch, n_tok),
                    lambda u, tc=tc, b=batch, t=n_tok: RB.tap_ln_bwd_tol(*tc, b, t, u),
                    lambda dt, tc=tc, b=batch, t=n_tok: _tap_torch(*tc, b, t, dt), tap32))
    ec = _eot_case(width)

    def eot32(ec=ec):
        rows = np.arange(3) * 7 + RR.eot_index(ec[2])
        o = np.zeros_like(ec[1])
        o[rows] = _ln_bwd32(ec[0], ec[1][rows], ec[3])
        return o
    out.append((f"eot_ln_bwd {width}", {"all": slice(None)}, RB.eot_ln_bwd(*ec), lambda u, ec=ec: RB.eot_ln_bwd_tol(*ec, u),
                lambda dt, ec=ec: _eot_torch(*ec, dt), eot32))
    dy, dyg, x = RB.l2_bwd_inputs(width)
    for name, d, group, scale in (("rows", dy, 0, 1.0), ("group 5", dyg, 5, 1 / 5)):
        out.append((f"l2_normalize_bwd {width} {name}", RB.L2_FAMILY_ROWS, RB.l2_normalize_bwd(d, x, group, scale),
                    lambda u, a=(d, x, group, scale): RB.l2_bwd_tol(*a, u),
                    lambda dt, a=(d, x, group, scale): _l2_torch(*a, dt), lambda a=(d, x, group, scale): _l2_bwd32(*a)))
    for aw in (0.1, 1.0, 0.0):
        dy, x, u_ = RB.blend_bwd_inputs(15, width)
        for k, part in enumerate(("dx", "du")):
            out.append((f"blend_bwd {part} {width} aw {aw}", BLEND_FAMILY_ROWS,
                        RB.blend_bwd(dy, x, u_, aw)[k], lambda u, a=(dy, x, u_, aw), k=k: RB.blend_bwd_tol(*a, u)[k],
                        lambda dt, a=(dy, x, u_, aw), k=k: _blend_torch(*a, dt)[k],
                        lambda a=(dy, x, u_, aw), k=k: _blend_bwd32(*a)[k]))
    return out


def _check_case(name, fams, ref, tol, torch_impl, numpy32):
    """The reference against float64 autograd, then both float32 implementations against half the bound."""
    t64, t32 = tol(RB.U64), tol(RB.U)
    assert ref.dtype == np.float64 and t32.shape == ref.shape and np.all(t32 >= 0)
    w64 = _worst(torch_impl(torch.float64), ref, t64)
    print(f"{name}: float64 autograd, worst |difference| / bound(u = 2^-53) = {w64:.3f}")
    assert w64 <= F64_MULT, name
    for impl, got in (("torch float32 autograd", torch_impl(torch.float32)), ("numpy float32, kernel order", numpy32())):
        assert got.dtype == F32
        for fam, rows in fams.items():
            w = _worst(got[rows], ref[rows], t32[rows])
            print(f"{name} {fam}: {impl}, worst |error| / bound = {w:.3f}, slack {1 / w if w else np.inf:.1f}")
            assert w <= 0.5, (name, fam, impl)


@pytest.mark.parametrize("width", WIDTHS)
def test_row_references_agree_with_autograd_and_leave_float32_a_factor_of_two(width):
    """layer_norm_bwd (every rows_ref.ln_inputs family), tap_ln_bwd (n_tok 5 and 2), eot_ln_bwd (EOT first,
    last, twice), l2_normalize_bwd (per row and group 5; ordinary, zero, 1e-13 and 1e-11 rows) and
    blend_bwd (aw 0.1, 1, 0; norm ratios 1e-3 .. 1e3): equal to float64 autograd within F64_MULT times
    the bound at u = 2^-53, and both float32 implementations within half the float32 bound on every
    family and element."""
    for case in _cases(width):
        _check_case(*case)


@pytest.mark.parametrize("n", RB.ANCHOR_NS)
def test_anchor_reference_agrees_with_autograd_and_leaves_float32_a_factor_of_two(n):
    for dim in RB.ANCHOR_DIMS:
        e, g = RB.anchor_bwd_inputs(n, dim)
        _check_case(f"anchor_reduce_bwd n {n} dim {dim}", {"all": slice(None)}, RB.anchor_reduce_bwd(e, g),
                    lambda u: RB.anchor_bwd_tol(e, g, u), lambda dt: _anchor_torch(e, g, dt), lambda: _anchor_bwd32(e, g))


@pytest.mark.parametrize("N,K", RB.WGRAD_NKS)
def test_wgrad_reference_agrees_with_autograd_and_leaves_float32_a_factor_of_two(N, K):
    """Also: on the integer inputs both float32 implementations return the int64 product exactly."""
    for M in RB.WGRAD_MS:
        dy, x = RB.wgrad_inputs(M, N, K)
        _check_case(f"linear_wgrad M {M} N {N} K {K}", {"all": slice(None)}, RB.linear_wgrad(dy, x),
                    lambda u: RB.wgrad_tol(dy, x, u), lambda dt: _wgrad_torch(dy, x, dt), lambda: _wgrad32(dy, x))
        dy, x = RB.wgrad_inputs(M, N, K, exact=True)
        exact = (dy.astype(np.int64).T @ x.astype(np.int64))
        assert np.abs(exact).max() < 2 ** 24 and M * 9 < 2 ** 24
        assert np.array_equal(_wgrad32(dy, x), exact.astype(F32)) and np.array_equal(RB.linear_wgrad(dy, x), exact)


# ---------------------------------------------------------------------------- the bounds refuse wrong formulas
def _report(name, mutant, ref, tol, fams, require=True):
    worst = {fam: _worst(mutant[rows], ref[rows], tol[rows]) for fam, rows in fams.items()}
    print(f"{name}: exceeds the bound by " + ", ".join(f"{fam} {w:.3g}" for fam, w in worst.items()))
    # over 2: a kernel computing this formula with a rounding error of its own inside the bound still fails
    assert max(worst.values()) > 2 or not require, name


@pytest.mark.parametrize("width", WIDTHS)
def test_bounds_refuse_the_wrong_formulas(width):
    """Each wrong formula, in float64, against the float32 bound; the factor per family is printed."""
    ALL = {"all": slice(None)}
    dy, x, w = (RR.f64(a) for a in RB.ln_bwd_inputs(width))
    ref, tol = RB.layer_norm_bwd(dy, x, w), RB.ln_bwd_tol(dy, x, w)
    g, xh, rstd, s1, s2 = RB._ln_parts(dy, x, w)
    fams = RR.LN_FAMILY_ROWS
    _report(f"LN bwd without mean(g) {width}", rstd * (g - xh * s2), ref, tol, fams)
    _report(f"LN bwd without xh mean(g xh) {width}", rstd * (g - s1), ref, tol, fams)
    d = x - x.mean(-1, keepdims=True)
    rs_u = 1.0 / np.sqrt((d * d).sum(-1, keepdims=True) / (width - 1) + 1e-5)
    xh_u = d * rs_u
    _report(f"LN bwd with unbiased variance {width}", rs_u * (g - s1 - xh_u * (g * xh_u).mean(-1, keepdims=True)),
            ref, tol, fams)
    _report(f"LN bwd with w after the projection {width}",
            w * rstd * (dy - dy.mean(-1, keepdims=True) - xh * (dy * xh).mean(-1, keepdims=True)), ref, tol, fams)

    dyr, dyg, x = RB.l2_bwd_inputs(width)
    ref, tol = RB.l2_normalize_bwd(dyr, x), RB.l2_bwd_tol(dyr, x)
    x64 = RR.f64(x)
    n = np.sqrt((x64 * x64).sum(-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        y = x64 / n
        proj = (RR.f64(dyr) - y * (y * RR.f64(dyr)).sum(-1, keepdims=True)) / n
        _report(f"l2 bwd without the projection {width}", np.where(n > 1e-12, RR.f64(dyr) / n, RR.f64(dyr) / 1e-12),
                ref, tol, RB.L2_FAMILY_ROWS)
    _report(f"l2 bwd with the clamp at 1e-6 {width}", np.where(n > 1e-6, proj, RR.f64(dyr) / 1e-6), ref, tol,
            RB.L2_FAMILY_ROWS)
    ref, tol = RB.l2_normalize_bwd(dyg, x, 5, 1 / 5), RB.l2_bwd_tol(dyg, x, 5, 1 / 5)
    shifted = np.minimum((np.arange(15) + 1) // 5, 2)
    _report(f"l2 bwd with the group broadcast dy[(r + 1) // group] {width}", RB.l2_normalize_bwd(dyg[shifted], x, 0, 1 / 5),
            ref, tol, RB.L2_FAMILY_ROWS)

    dy, x, u_ = RB.blend_bwd_inputs(15, width)
    _report(f"blend bwd without the path through |x| {width}", (1.0 - float(F32(0.1))) * RR.f64(dy),
            RB.blend_bwd(dy, x, u_, 0.1)[0], RB.blend_bwd_tol(dy, x, u_, 0.1)[0], BLEND_FAMILY_ROWS)

    for n_tok in (5, 2):
        dtap, x, w, g = _tap_case(width, 3, n_tok)
        # dtap[b, t], wrapped inside the image
        wrong = np.roll(dtap.reshape(3, n_tok - 1, width), -1, axis=1).reshape(dtap.shape)
        if n_tok == 2:
            wrong = np.roll(dtap, -1, axis=0)  # one tap row per image: dtap[b, t] is the next image's
        _report(f"tap_ln_bwd reading dtap[b, t] {width} n_tok {n_tok}", RB.tap_ln_bwd(wrong, x, w, g, 3, n_tok),
                RB.tap_ln_bwd(dtap, x, w, g, 3, n_tok), RB.tap_ln_bwd_tol(dtap, x, w, g, 3, n_tok), ALL)

    if width == WIDTHS[0]:
        for M in (64, 65, 129):
            dy, x = RB.wgrad_inputs(M, 64, 192)
            keep = np.arange(M) % RB.WGRAD_ROWS != RB.WGRAD_ROWS - 1
            _report(f"linear_wgrad dropping the last row of each 64-row chunk M {M}", RB.linear_wgrad(dy[keep], x[keep]),
                    RB.linear_wgrad(dy, x), RB.wgrad_tol(dy, x), ALL)
        for n in RB.ANCHOR_NS:
            for dim in RB.ANCHOR_DIMS:
                e, g = RB.anchor_bwd_inputs(n, dim)
                e64, g64 = RR.f64(e), RR.f64(g)
                en = np.sqrt((e64 * e64).sum(-1, keepdims=True))
                eh = e64 / en
                m = eh.mean(0)
                dmn = g64 / np.linalg.norm(m) / n  # the outer normalisation's projection dropped
                _report(f"anchor_reduce_bwd without the outer projection n {n} dim {dim}",
                        (dmn - eh * (eh * dmn).sum(-1, keepdims=True)) / en, RB.anchor_reduce_bwd(e, g),
                        RB.anchor_bwd_tol(e, g), ALL, require=n > 1)  # n = 1: the inner projection removes the same part


# ---------------------------------------------------------------------------- wrapper rejections (no device)
def test_overlap_is_exact_for_column_views_and_row_shifts():
    buf = torch.zeros(16, 40)
    a, b, c = buf[:, :16], buf[:, 16:32], buf[:, 12:28]
    assert not ops._overlap(a, b) and not ops._overlap(b, a)          # two column views of one buffer
    assert ops._overlap(a, c) and ops._overlap(c, b) and ops._overlap(a, a)
    assert ops._overlap(buf[1:, :16], buf[:-1, :16])                  # the same columns, one row down
    assert not ops._overlap(buf[:8], buf[8:]) and ops._overlap(buf[:9], buf[8:])
    assert not ops._overlap(buf[:, 36:], buf[:, :4]) and not ops._overlap(buf[3:4, 4:8], buf[:, :4])
    assert ops._overlap(buf[3:4, 3:8], buf[:, :4]) and ops._overlap(buf[15:, 39:], buf.view(-1)[-1:])
    assert ops._overlap(buf[:, :16], torch.as_strided(buf, (8, 16), (80, 1), 16))  # other stride: by range
    assert not ops._overlap(buf[:, :0], buf)


def test_bwd_wrappers_reject_overlapping_operands_without_a_launch():
    """Before this test the wrappers compared start addresses only: an output one row or a few columns
    away from an input it must not share memory with reached the launch, where one wave writes what
    another still reads. CPU tensors: a call that passes the checks ends in _dev's RuntimeError."""
    W_ = 768
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)  # noqa: E731

    def passes(fn):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()

    def rejected(fn):
        with pytest.raises(ValueError, match="overlaps"):
            fn()

    big = z(17, 2 * W_)
    lo, hi, down, shifted = big[:15, :W_], big[:15, W_:], big[1:16, :W_], big[:15, 4:W_ + 4]
    w, other = z(W_), z(15, W_)
    # layernorm_bwd: out never x; dy / residual only as the same view
    passes(lambda: ops.layernorm_bwd(other, lo, w, out=hi))                      # column views side by side
    passes(lambda: ops.layernorm_bwd(hi, other, w, residual=hi, out=hi))
    for bad in (down, shifted):
        rejected(lambda: ops.layernorm_bwd(other, lo, w, out=bad))
        rejected(lambda: ops.layernorm_bwd(lo, other, w, out=bad))
        rejected(lambda: ops.layernorm_bwd(other, z(15, W_), w, residual=lo, out=bad))
    rejected(lambda: ops.layernorm_bwd(other, lo, w, out=lo))
    # l2_normalize_bwd: the same, and never dy under a group
    passes(lambda: ops.l2_normalize_bwd(hi, lo, out=hi))
    for bad in (down, shifted):
        rejected(lambda: ops.l2_normalize_bwd(other, lo, out=bad))
        rejected(lambda: ops.l2_normalize_bwd(lo, other, out=bad))
    rejected(lambda: ops.l2_normalize_bwd(big[12:15, :W_], other, group=5, scale=0.2, out=lo))
    rejected(lambda: ops.l2_normalize_bwd(big[:3, :W_], other, group=5, scale=0.2, out=lo))
    # the contiguous ones: one row down inside one allocation
    flat = z(17, W_)
    up, dn = flat[:15], flat[1:16]
    rejected(lambda: ops.adapter_blend_bwd(other, up, z(15, W_), 0.1, dx=dn))
    rejected(lambda: ops.adapter_blend_bwd(up, other, z(15, W_), 0.1, dx=dn))
    rejected(lambda: ops.adapter_blend_bwd(up, other, z(15, W_), 0.1, dx=up, du=dn))
    passes(lambda: ops.adapter_blend_bwd(up, other, z(15, W_), 0.1, dx=up))
    rejected(lambda: ops.tap_ln_bwd(z(12, W_), up, w, dn, 3, 5))
    rejected(lambda: ops.tap_ln_bwd(flat[2:14], other, w, up, 3, 5))
    tok = z(3, 5, dt=torch.int32)
    rejected(lambda: ops.eot_ln_bwd(z(3, W_), up, tok, w, out=dn))
    rejected(lambda: ops.eot_ln_bwd(flat[14:17], other, tok, w, out=up))
    rejected(lambda: ops.anchor_reduce_bwd(up, z(W_, 2), 0, out=dn))
    # linear_wgrad: dW against dY, X and the workspace; the workspace against dY and X
    sq = z(130, 64)
    ws = z(2 * 64 * 64)
    passes(lambda: ops.linear_wgrad(sq[:64], z(64, 64), out=z(64, 64), workspace=ws))
    rejected(lambda: ops.linear_wgrad(sq[:64], z(64, 64), out=sq[1:65], workspace=ws))
    rejected(lambda: ops.linear_wgrad(z(64, 64), sq[:64], out=sq[63:127], workspace=ws))
    rejected(lambda: ops.linear_wgrad(z(64, 64), z(64, 64), out=ws[64:64 + 4096].view(64, 64), workspace=ws))
    rejected(lambda: ops.linear_wgrad(ws[:4096].view(64, 64), z(64, 64), out=z(64, 64), workspace=ws))
    rejected(lambda: ops.linear_wgrad(z(64, 64), ws[4096:].view(64, 64), out=z(64, 64), workspace=ws))
