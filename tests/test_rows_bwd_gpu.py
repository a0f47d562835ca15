"""The backward row kernels (aa-clip_amd/csrc/text_bwd.hip, visual_bwd.hip) on their own, against the
float64 restatements of tests/rows_bwd_ref.py: layernorm_bwd, tap_ln_bwd, l2_normalize_bwd,
adapter_blend_bwd, eot_ln_bwd, anchor_reduce_bwd and linear_wgrad.

One wave owns a row and a 256-thread workgroup four rows, so the row kernels run at 3 images of 5
tokens (15 rows: a ragged last workgroup, workgroups that straddle images) and at one row, at both
widths (768 -> VEC 3, 1024 -> VEC 4, the instantiation stage 2 uses). Every comparison is per element
against the float64 reference with the a priori bound of rows_bwd_ref (checked against two float32
CPU implementations and a list of wrong formulas in tests/test_rows_bwd_host.py, never fitted to the
kernels); what has no ordering freedom is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

from aaclip import ops

import rows_bwd_ref as RB
import rows_ref as RR
from test_rows_gpu import SENTINEL, _same_bits, _t, _within

pytestmark = pytest.mark.gpu

WIDTHS = (768, 1024)
B, NT = 3, 5
ROWS = B * NT
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _ln_case(width):
    return RB.ln_bwd_inputs(width)


def _padded(a, dev, ld, off, fill):
    """(buffer [rows, ld] of `fill`, its column view [:, off:off + width] holding a): a strided operand whose
    row starts are 16-byte aligned."""
    rows, width = a.shape
    buf = torch.full((rows, ld), fill, device=dev)
    view = buf[:, off:off + width]
    view.copy_(_t(a, dev))
    assert ld % 4 == 0 and view.data_ptr() % 16 == 0 and not view.is_contiguous()
    return buf, view


def _pad_intact(buf, off, width, fill):
    want = torch.full_like(buf, fill)
    return _same_bits(buf[:, :off], want[:, :off]) and _same_bits(buf[:, off + width:], want[:, off + width:])


def _nan_rows(t):
    return torch.isnan(t).all(-1).cpu().numpy()


# ---------------------------------------------------------------------------- layernorm_bwd
@pytest.mark.parametrize("rows", [ROWS, 1])
@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_bwd_input_families(dev, width, rows):
    """Closes "layernorm_bwd inputs are only randn * 2 + 0.3", "width 1024 is never run directly" and "the
    comparison is one relative L2 norm": every rows_ref.ln_inputs family (mean 100, an outlier channel,
    scale 1e-4, constant, zero) with a non-trivial w, each element against ln_bwd_tol."""
    dy, x, w = _ln_case(width)
    fams = RR.LN_FAMILY_ROWS
    if rows == 1:
        dy, x, fams = dy[7:8], x[7:8], {"outlier": slice(0, 1)}
    ref, tol = RB.layer_norm_bwd(dy, x, w), RB.ln_bwd_tol(dy, x, w)
    out = torch.full((rows, width), NAN, device=dev)
    ops.layernorm_bwd(_t(dy, dev), _t(x, dev), _t(w, dev), out=out)
    for fam, r in fams.items():
        _within(out[r], ref[r], tol[r], f"layernorm_bwd {rows}x{width} {fam}")


@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_bwd_strided_rows_and_sentinel(dev, width):
    """Closes "row strides are never tested": dy, x, residual and out are column views of padded buffers with
    four different row strides; the bits of the contiguous call, out's padding intact, 1e30 in the
    inputs' padding without effect."""
    dy, x, w = _ln_case(width)
    res = np.random.default_rng(width).standard_normal(x.shape).astype(np.float32)
    wd = _t(w, dev)
    _, dyv = _padded(dy, dev, width + 8, 4, 1e30)
    _, xv = _padded(x, dev, 2 * width + 12, width + 8, 1e30)
    _, rv = _padded(res, dev, width + 4, 0, 1e30)
    ob, ov = _padded(np.full(x.shape, SENTINEL, np.float32), dev, width + 16, 8, SENTINEL)
    assert len({t.stride(0) for t in (dyv, xv, rv, ov)}) == 4
    ops.layernorm_bwd(dyv, xv, wd, residual=rv, out=ov)
    oc = ops.layernorm_bwd(_t(dy, dev), _t(x, dev), wd, residual=_t(res, dev))
    assert _same_bits(ov, oc) and _pad_intact(ob, 8, width, SENTINEL)
    ref = RB.layer_norm_bwd(dy, x, w) + RR.f64(res)
    _within(ov, ref, RB.ln_bwd_tol(dy, x, w) + RB.U * np.abs(ref), f"strided layernorm_bwd {width}")


@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_bwd_aliasing_forms(dev, width):
    """Closes the aliasing half of "row strides are never tested": residual is out (the engine's form), dy is
    out, and all distinct give the same bits."""
    dy, x, w = _ln_case(width)
    res = np.random.default_rng(width + 1).standard_normal(x.shape).astype(np.float32)
    dyd, xd, wd, rd = _t(dy, dev), _t(x, dev), _t(w, dev), _t(res, dev)
    apart = ops.layernorm_bwd(dyd, xd, wd, residual=rd, out=torch.full((ROWS, width), NAN, device=dev))
    r2 = rd.clone()
    assert ops.layernorm_bwd(dyd, xd, wd, residual=r2, out=r2) is r2 and _same_bits(r2, apart)
    d2 = dyd.clone()
    assert ops.layernorm_bwd(d2, xd, wd, residual=rd, out=d2) is d2 and _same_bits(d2, apart)
    d3 = dyd.clone()
    ops.layernorm_bwd(d3, xd, wd, out=d3)  # no residual
    assert _same_bits(d3, ops.layernorm_bwd(dyd, xd, wd))
    ref = RB.layer_norm_bwd(dy, x, w) + RR.f64(res)
    _within(apart, ref, RB.ln_bwd_tol(dy, x, w) + RB.U * np.abs(ref), f"layernorm_bwd + residual {width}")


@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_bwd_nan_stays_in_its_row(dev, width):
    """Closes "nothing checks that a NaN stays in its row": one NaN in x or in dy of row 5 (second wave of the
    second workgroup) makes exactly that row NaN, every other row keeps its bits."""
    dy, x, w = _ln_case(width)
    dyd, xd, wd = _t(dy, dev), _t(x, dev), _t(w, dev)
    clean = ops.layernorm_bwd(dyd, xd, wd)
    for which in ("x", "dy"):
        a, b = dyd.clone(), xd.clone()
        (b if which == "x" else a)[5, 301] = NAN
        got = ops.layernorm_bwd(a, b, wd)
        assert list(np.flatnonzero(_nan_rows(got))) == [5] and not torch.isnan(got[[4, 6]]).any(), which
        keep = [r for r in range(ROWS) if r != 5]
        assert _same_bits(got[keep], clean[keep]), which


# ---------------------------------------------------------------------------- tap_ln_bwd
def _tap_case(width, n_tok):
    rng = np.random.default_rng(11 * width + n_tok)
    x, w, _ = RR.ln_inputs(width, seed=2)
    x = x[:B * n_tok]
    dtap = rng.standard_normal((B * (n_tok - 1), width)).astype(np.float32)
    g = rng.standard_normal((B * n_tok, width)).astype(np.float32)
    g[::n_tok] = SENTINEL
    return dtap, x, w, g


@pytest.mark.parametrize("n_tok", [NT, 2])
@pytest.mark.parametrize("width", WIDTHS)
def test_tap_ln_bwd_accumulates_onto_g(dev, width, n_tok):
    """Closes "tap_ln_bwd at n_tok = 2": (batch, n_tok) = (3, 5) and (3, 2) on a non-zero g whose CLS rows
    hold the sentinel: those keep their bits, every token row is g + LN_bwd within tap_ln_bwd_tol."""
    dtap, x, w, g = _tap_case(width, n_tok)
    gd = _t(g, dev)
    assert ops.tap_ln_bwd(_t(dtap, dev), _t(x, dev), _t(w, dev), gd, B, n_tok) is gd
    assert _same_bits(gd[::n_tok], torch.full((B, width), SENTINEL, device=dev))
    _within(gd, RB.tap_ln_bwd(dtap, x, w, g, B, n_tok), RB.tap_ln_bwd_tol(dtap, x, w, g, B, n_tok),
            f"tap_ln_bwd {B}x{n_tok}x{width}")


@pytest.mark.parametrize("n_tok", [NT, 2])
@pytest.mark.parametrize("width", WIDTHS)
def test_tap_ln_bwd_row_mapping(dev, width, n_tok):
    """Closes "its (b, t - 1) row mapping pinned": with dtap zero except tap row k, exactly the row (b, t) of g
    with b (n_tok - 1) + t - 1 == k changes, for every k."""
    dtap, x, w, g = _tap_case(width, n_tok)
    xd, wd = _t(x, dev), _t(w, dev)
    for k in range(B * (n_tok - 1)):
        one = np.zeros_like(dtap)
        one[k] = dtap[k]
        gd = _t(g, dev)
        ops.tap_ln_bwd(_t(one, dev), xd, wd, gd, B, n_tok)
        changed = np.flatnonzero((gd.cpu().numpy().view(np.int32) != g.view(np.int32)).any(-1))
        b, t = k // (n_tok - 1), k % (n_tok - 1) + 1
        assert list(changed) == [b * n_tok + t], (k, changed)


# ---------------------------------------------------------------------------- l2_normalize_bwd
@pytest.mark.parametrize("group", [0, 5])
@pytest.mark.parametrize("width", WIDTHS)
def test_l2_normalize_bwd_branches_and_groups(dev, width, group):
    """Closes "the clamp branch of l2_normalize_bwd near 1e-12" and the per-row comparison: row norms of 0 and
    1e-13 (clamp branch), 1e-11 (regular branch) beside ordinary rows from 3e-2 to 3e4, per row and with
    group = 5, scale = 1 / 5 (the groups straddle the 4-row workgroups); for ordinary rows dx . x is
    within the bound of zero."""
    dyr, dyg, x = RB.l2_bwd_inputs(width)
    dy, scale = (dyg, 1 / 5) if group else (dyr, 1.0)
    ref, tol = RB.l2_normalize_bwd(dy, x, group, scale), RB.l2_bwd_tol(dy, x, group, scale)
    out = torch.full((ROWS, width), NAN, device=dev)
    ops.l2_normalize_bwd(_t(dy, dev), _t(x, dev), group=group, scale=scale, out=out)
    for fam, r in RB.L2_FAMILY_ROWS.items():
        _within(out[r], ref[r], tol[r], f"l2_normalize_bwd {width} group {group} {fam}")
    r = RB.L2_FAMILY_ROWS["ordinary"]
    x64 = RR.f64(x)[r]
    dot, bound = np.abs((RR.f64(out)[r] * x64).sum(-1)), (tol[r] * np.abs(x64)).sum(-1)
    print(f"l2_normalize_bwd {width} group {group}: worst |dx . x| / bound {np.max(dot / bound):.3f}")
    assert np.all(dot <= bound)


@pytest.mark.parametrize("width", WIDTHS)
def test_l2_normalize_bwd_strided_and_in_place(dev, width):
    """Closes "the engine passes non-contiguous raw column views to l2_normalize_bwd": dy, x and out are
    column views with three row strides, the bits of the contiguous call, sentinels intact; then out is
    dy at equal stride, contiguous and as a view."""
    dy, _, x = RB.l2_bwd_inputs(width)
    oc = ops.l2_normalize_bwd(_t(dy, dev), _t(x, dev))
    dyb, dyv = _padded(dy, dev, width + 12, 8, SENTINEL)
    _, xv = _padded(x, dev, 4 * 768 + width, 4 * 768, 1e30)  # the engines' segbuf offset
    ob, ov = _padded(np.full(x.shape, SENTINEL, np.float32), dev, width + 4, 4, SENTINEL)
    ops.l2_normalize_bwd(dyv, xv, out=ov)
    assert _same_bits(ov, oc) and _pad_intact(ob, 4, width, SENTINEL)
    assert ops.l2_normalize_bwd(dyv, xv, out=dyv) is dyv
    assert _same_bits(dyv, oc) and _pad_intact(dyb, 8, width, SENTINEL)
    d2 = _t(dy, dev)
    ops.l2_normalize_bwd(d2, xv, out=d2)
    assert _same_bits(d2, oc)


# ---------------------------------------------------------------------------- adapter_blend_bwd
@pytest.mark.parametrize("aw", [0.1, 1.0])
@pytest.mark.parametrize("rows", [ROWS, 1])
@pytest.mark.parametrize("width", WIDTHS)
def test_adapter_blend_bwd_against_float64(dev, width, rows, aw):
    """Closes "width 1024 is never run directly" and the per-row comparison for the blend: norm ratios |x| / |u|
    from 1e-3 to 1e3 (the one-row case takes the first, 1e-3), dx and du per element; dx written over
    dy gives the out-of-place bits."""
    dy, x, u = (a[:rows] for a in RB.blend_bwd_inputs(ROWS, width))
    dyd, xd, ud = _t(dy, dev), _t(x, dev), _t(u, dev)
    dx = torch.full((rows, width), NAN, device=dev)
    du = torch.full((rows, width), NAN, device=dev)
    ops.adapter_blend_bwd(dyd, xd, ud, aw, dx=dx, du=du)
    rx, ru = RB.blend_bwd(dy, x, u, aw)
    tx, tu = RB.blend_bwd_tol(dy, x, u, aw)
    _within(dx, rx, tx, f"adapter_blend_bwd dx {rows}x{width} aw {aw}")
    _within(du, ru, tu, f"adapter_blend_bwd du {rows}x{width} aw {aw}")
    g = dyd.clone()
    dx2, du2 = ops.adapter_blend_bwd(g, xd, ud, aw, dx=g)
    assert dx2 is g and _same_bits(g, dx) and _same_bits(du2, du)


@pytest.mark.parametrize("width", WIDTHS)
def test_adapter_blend_bwd_zero_weight_and_nan_rows(dev, width):
    """Closes "adapter_blend_bwd at aw = 0" and NaN isolation: at aw = 0 dx has dy's bits and du is exactly
    zero; one NaN in x or dy of row 5 makes exactly that row of dx and du NaN, the others keep their bits."""
    dy, x, u = RB.blend_bwd_inputs(ROWS, width)
    dyd, xd, ud = _t(dy, dev), _t(x, dev), _t(u, dev)
    dx, du = ops.adapter_blend_bwd(dyd, xd, ud, 0.0)
    assert _same_bits(dx, dyd) and bool((du == 0).all())
    dx, du = ops.adapter_blend_bwd(dyd, xd, ud, 0.1)
    keep = [r for r in range(ROWS) if r != 5]
    for which in ("x", "dy"):
        a, b = dyd.clone(), xd.clone()
        (b if which == "x" else a)[5, 301] = NAN
        nx, nu = ops.adapter_blend_bwd(a, b, ud, 0.1)
        for got, clean in ((nx, dx), (nu, du)):
            assert list(np.flatnonzero(_nan_rows(got))) == [5] and not torch.isnan(got[keep]).any(), which
            assert _same_bits(got[keep], clean[keep]), which


# ---------------------------------------------------------------------------- eot_ln_bwd
@pytest.mark.parametrize("ctx", [7, 77])
@pytest.mark.parametrize("width", WIDTHS)
def test_eot_ln_bwd_positions_and_ties(dev, width, ctx):
    """Closes "eot_ln_bwd with a tie in the token ids" and width 1024: EOT at the first position, at the last,
    and twice in one sequence (in two lanes, and at ctx 77 also twice in lane 6's stride): the first
    occurrence takes the gradient, every other row is exactly zero over a NaN-filled out."""
    eot = 49407
    spots = [(0,), (ctx - 1,), (2, 5)] + ([(6, 70)] if ctx > 70 else [])
    tok = np.stack([(np.arange(ctx, dtype=np.int32) * 7 + k) % 40 + 1 for k in range(len(spots))])
    for s, p in enumerate(spots):
        tok[s, list(p)] = eot
    n = len(spots)
    rng = np.random.default_rng(ctx + width)
    x = (rng.standard_normal((n * ctx, width)) * 2 + 0.3).astype(np.float32)
    dy = rng.standard_normal((n, width)).astype(np.float32)
    w = _ln_case(width)[2]
    out = torch.full((n * ctx, width), NAN, device=dev)
    ops.eot_ln_bwd(_t(dy, dev), _t(x, dev), _t(tok, dev), _t(w, dev), out=out)
    first = np.arange(n) * ctx + np.array([p[0] for p in spots])
    nonzero = np.flatnonzero((out != 0).any(-1).cpu().numpy())
    assert list(nonzero) == list(first), (nonzero, first)
    other = np.setdiff1d(np.arange(n * ctx), first)
    assert _same_bits(out[other], torch.zeros(len(other), width, device=dev))
    _within(out, RB.eot_ln_bwd(dy, x, tok, w), RB.eot_ln_bwd_tol(dy, x, tok, w), f"eot_ln_bwd {n}x{ctx}x{width}")


# ---------------------------------------------------------------------------- anchor_reduce_bwd
@pytest.mark.parametrize("dim", RB.ANCHOR_DIMS)
@pytest.mark.parametrize("n", RB.ANCHOR_NS)
def test_anchor_reduce_bwd(dev, n, dim):
    """Closes "anchor_reduce_bwd is run only at dim 768, n in {1, 6, 10}, ncols = 2, col = 1": dims that are no
    multiple of 256 (m_local's ragged last column group), dim 1024, n = 256 (all of inv_norm), columns
    (ncols, col) = (1, 0), (3, 0), (3, 2) with 1e30 in the other columns of dT; two launches give the same
    bits; demb_s . emb_s is within the bound of zero (the gradient of a normalised vector)."""
    e, g = RB.anchor_bwd_inputs(n, dim)
    ref, tol = RB.anchor_reduce_bwd(e, g), RB.anchor_bwd_tol(e, g)
    ed = _t(e, dev)
    outs = []
    for ncols, col in ((1, 0), (3, 0), (3, 2)):
        dT = torch.full((dim, ncols), 1e30, device=dev)
        dT[:, col] = _t(g, dev)
        out = torch.full((n, dim), NAN, device=dev)
        ops.anchor_reduce_bwd(ed, dT, col, out=out)
        assert _same_bits(out, ops.anchor_reduce_bwd(ed, dT, col))
        outs.append(out)
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
    _within(outs[0], ref, tol, f"anchor_reduce_bwd n={n} dim={dim}")
    e64 = RR.f64(e)
    dot, bound = np.abs((RR.f64(outs[0]) * e64).sum(-1)), (tol * np.abs(e64)).sum(-1)
    print(f"anchor_reduce_bwd n={n} dim={dim}: worst |demb . emb| / bound {np.max(dot / bound):.3f}")
    assert np.all(dot <= bound)


# ---------------------------------------------------------------------------- linear_wgrad
@pytest.mark.parametrize("N,K", RB.WGRAD_NKS)
@pytest.mark.parametrize("M", RB.WGRAD_MS)
def test_linear_wgrad_chunk_edges(dev, M, N, K):
    """Closes "linear_wgrad misses its chunk edges": M at the 16-row staging pass (15 / 16 / 17) and the
    64-row chunk edges (63 / 64 / 65, 128 / 129), one and three tiles along N and along K. Integer
    operands in -3 .. 3 must give the int64 product bit for bit (every row, chunk and tile index, no
    tolerance); normal operands stay within wgrad_tol."""
    dy, x = RB.wgrad_inputs(M, N, K, exact=True)
    exact = dy.astype(np.int64).T @ x.astype(np.int64)
    assert np.abs(exact).max() < 2 ** 24
    got = torch.full((N, K), NAN, device=dev)
    ops.linear_wgrad(_t(dy, dev), _t(x, dev), out=got)
    assert _same_bits(got.cpu(), torch.from_numpy(exact.astype(np.float32))), f"linear_wgrad M {M} N {N} K {K}: not exact"
    dy, x = RB.wgrad_inputs(M, N, K)
    _within(ops.linear_wgrad(_t(dy, dev), _t(x, dev)), RB.linear_wgrad(dy, x), RB.wgrad_tol(dy, x),
            f"linear_wgrad M {M} N {N} K {K}")


@pytest.mark.parametrize("N,K", RB.WGRAD_NKS)
@pytest.mark.parametrize("M", RB.WGRAD_MS)
def test_linear_wgrad_strided_operands_and_workspace(dev, M, N, K):
    """Closes "never run: a strided dY, X or dW, or a caller-supplied workspace": dY and X are column slices
    (odd offsets and strides: the entry asks for 4-byte alignment only) of buffers otherwise 1e30, dW a
    column view of a sentinel buffer that stays intact, all with the contiguous call's bits; a larger,
    NaN-filled workspace gives the same bits, holds no NaN in the ceil(M / 64) N K partials the finalize
    pass reads and only NaN beyond them."""
    dy, x = RB.wgrad_inputs(M, N, K)
    dyd, xd = _t(dy, dev), _t(x, dev)
    plain = ops.linear_wgrad(dyd, xd)
    yb = torch.full((M, N + 67), 1e30, device=dev)
    xb = torch.full((M, 2 * K + 5), 1e30, device=dev)
    yv, xv = yb[:, 3:3 + N], xb[:, K + 1:2 * K + 1]
    yv.copy_(dyd)
    xv.copy_(xd)
    wb = torch.full((N, K + 9), SENTINEL, device=dev)
    wv = wb[:, 2:2 + K]
    assert ops.linear_wgrad(yv, xv, out=wv) is wv
    assert _same_bits(wv, plain) and _pad_intact(wb, 2, K, SENTINEL)
    need = ops.linear_wgrad_workspace(M, N, K, dev).numel()
    assert need == -(-M // RB.WGRAD_ROWS) * N * K
    ws = torch.full((need + 1000,), NAN, device=dev)
    assert _same_bits(ops.linear_wgrad(dyd, xd, workspace=ws), plain)
    assert not torch.isnan(ws[:need]).any() and bool(torch.isnan(ws[need:]).all())
