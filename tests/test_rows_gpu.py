"""The forward row kernels (aa-clip_amd/csrc/rows.hip) on their own, against the float64
restatements of tests/rows_ref.py: layernorm, embed_ln, block_tail, text_embed_ln, eot_ln,
l2_normalize, anchor_reduce and the im2col fallback, plus the ops wrappers' rejections.

One wave owns a row and a 256-thread workgroup four rows, so what can go wrong shows at a handful
of rows: B = 3 images of n_tok = 5 tokens (15 rows: a ragged last workgroup, workgroups that
straddle images) at both widths, and one case each at the product's own layouts (577 tokens at
1024, 77 at 768). The error bounds are rows_ref's (checked against float32 implementations in
tests/test_rows_host.py); every 16-bit / fp8 output is compared bit for bit with the same call's
fp32 output rounded once."""
import functools

import numpy as np
import pytest
import torch

from aaclip import ops

import rows_ref as RR

pytestmark = pytest.mark.gpu

WIDTHS = (768, 1024)
B, NT = 3, 5
ROWS = B * NT
DT16 = (torch.bfloat16, torch.float16)
DT3 = (torch.float32,) + DT16
FP8 = ops.FP8
SENTINEL = -7.25  # exact in every dtype used here


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _within(got, ref, tol, what):
    """Every element of got within tol of ref (a NaN fails); prints the worst error / bound."""
    err = np.abs(RR.f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / tol, 0.0)
    print(f"{what}: worst |error| {np.nanmax(err):.3e}, worst error / bound {np.nanmax(ratio):.3f}")
    ok = err <= tol
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} elements outside the bound, first at {np.argwhere(~ok)[0]}"


@functools.lru_cache(maxsize=None)
def _ln_inputs(width):
    return RR.ln_inputs(width)


def _ln_pair(width, seed):
    rng = np.random.default_rng(50 * seed + width)
    return ((1 + 0.1 * rng.standard_normal(width)).astype(np.float32),
            (0.1 * rng.standard_normal(width)).astype(np.float32))


def _dev_pair(p, dev):
    return (_t(p[0], dev), _t(p[1], dev))


# ---------------------------------------------------------------------------- layernorm
@pytest.mark.parametrize("rows", [ROWS, 1])
@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_fp32_against_float64(dev, width, rows):
    x, w, b = _ln_inputs(width)
    if rows == 1:
        x = x[7:8]  # an outlier-channel row
    ref = RR.layer_norm(x, w, b)
    y = torch.full((rows, width), float("nan"), device=dev)
    ops.layernorm(_t(x, dev), _t(w, dev), _t(b, dev), y)
    _within(y, ref, RR.ln_tol(x, w, ref), f"layernorm {rows}x{width}")


@pytest.mark.parametrize("dt", DT3)
@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_strided_rows_and_sentinel(dev, width, dt):
    """x and y are column views of padded buffers (ldx = 2 width + 8, ldy = width + 16): the same
    bits as the contiguous call, and nothing outside y's columns is written."""
    x, w, b = _ln_inputs(width)
    xb = torch.full((ROWS, 2 * width + 8), 1e30, device=dev)
    xv = xb[:, width + 8:]
    xv.copy_(_t(x, dev))
    yb = torch.full((ROWS, width + 16), SENTINEL, device=dev, dtype=dt)
    yv = yb[:, 8:8 + width]
    assert xv.data_ptr() % 16 == 0 and yv.data_ptr() % 16 == 0 and not xv.is_contiguous() and not yv.is_contiguous()
    wd, bd = _t(w, dev), _t(b, dev)
    ops.layernorm(xv, wd, bd, yv)
    yc = torch.empty(ROWS, width, device=dev, dtype=dt)
    ops.layernorm(_t(x, dev), wd, bd, yc)
    assert _same_bits(yv, yc)
    pad = torch.full((ROWS, 8), SENTINEL, device=dev, dtype=dt)
    assert _same_bits(yb[:, :8], pad) and _same_bits(yb[:, 8 + width:], pad)
    if dt == torch.float32:
        ref = RR.layer_norm(x, w, b)
        _within(yv, ref, RR.ln_tol(x, w, ref), f"strided layernorm {width}")


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_16bit_rounds_once(dev, width, dt):
    x, w, b = _ln_inputs(width)
    xd, wd, bd = _t(x, dev), _t(w, dev), _t(b, dev)
    y32 = torch.empty(ROWS, width, device=dev)
    y16 = torch.empty(ROWS, width, device=dev, dtype=dt)
    ops.layernorm(xd, wd, bd, y32)
    ops.layernorm(xd, wd, bd, y16)
    assert _same_bits(y16, y32.to(dt))


@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_nan_stays_in_its_row(dev, width):
    x, w, b = _ln_inputs(width)
    xd, wd, bd = _t(x, dev), _t(w, dev), _t(b, dev)
    y = torch.empty(ROWS, width, device=dev)
    ops.layernorm(xd, wd, bd, y)
    xn = xd.clone()
    xn[5, 301] = float("nan")  # row 5: second wave of the second workgroup
    yn = torch.empty(ROWS, width, device=dev)
    ops.layernorm(xn, wd, bd, yn)
    assert torch.isnan(yn[5]).all()
    keep = [r for r in range(ROWS) if r != 5]
    assert _same_bits(yn[keep], y[keep])


# ---------------------------------------------------------------------------- embed_ln
def _embed_case(batch, n_tok, width):
    rng = np.random.default_rng(17 * n_tok + width)
    rows = batch * n_tok
    x = rng.standard_normal((rows, width)).astype(np.float32)
    x[::n_tok] = np.nan  # the patch GEMM never writes the CLS rows
    cls = (0.5 * rng.standard_normal(width)).astype(np.float32)
    pos = (rng.standard_normal((n_tok, width)) * (1 + np.arange(n_tok) % 7)[:, None]).astype(np.float32)
    return x, cls, pos, _ln_pair(width, 1), _ln_pair(width, 2)


def _run_embed(dev, case, batch, n_tok, dt, h_sc=None):
    x, cls, pos, pre, ln1 = case
    X = _t(x, dev)
    H = torch.empty(X.shape, device=dev, dtype=dt)
    ops.embed_ln(X, _t(cls, dev), _t(pos, dev), _dev_pair(pre, dev), _dev_pair(ln1, dev), H, batch, n_tok, h_sc=h_sc)
    return X, H


@pytest.mark.parametrize("batch,n_tok,width", [(B, NT, 768), (B, NT, 1024), (2, 577, 1024)])
def test_embed_ln_against_float64(dev, batch, n_tok, width):
    """x = ln_pre(cls + pos[0] | x + pos[t]) and h = ln_1(x), each stage held to the single
    LayerNorm bound (h against the device's own x); 16-bit h is the fp32 h rounded once."""
    case = _embed_case(batch, n_tok, width)
    x, cls, pos, pre, ln1 = case
    X, H = _run_embed(dev, case, batch, n_tok, torch.float32)
    e = RR.embed_rows(x, cls, pos, n_tok)
    ref = RR.layer_norm(e, *pre)
    _within(X, ref, RR.ln_tol(e, pre[0], ref), f"embed_ln x {batch}x{n_tok}x{width}")
    x_out = RR.f64(X)
    ref = RR.layer_norm(x_out, *ln1)
    _within(H, ref, RR.ln_tol(x_out, ln1[0], ref), f"embed_ln h {batch}x{n_tok}x{width}")
    for dt in DT16:
        X16, H16 = _run_embed(dev, case, batch, n_tok, dt)
        assert _same_bits(X16, X) and _same_bits(H16, H.to(dt)), dt


@pytest.mark.parametrize("width", WIDTHS)
def test_embed_ln_mx_output(dev, width):
    """fp8 MX h: the bytes and the e8m0 scales equal quant_fp8_mx of the fp32 h; the scale buffer's
    ld exceeds the row count and its other rows stay untouched."""
    case = _embed_case(B, NT, width)
    X, H = _run_embed(dev, case, B, NT, torch.float32)
    ld = ROWS + 9
    q_ref = torch.empty(ROWS, width, device=dev, dtype=FP8)
    s_ref = ops.mx_scales(ROWS, width, dev, ld=ld).fill_(0x5A)
    ops.quant_fp8_mx(H, q_ref, s_ref)
    s = ops.mx_scales(ROWS, width, dev, ld=ld).fill_(0x5A)
    X8, q = _run_embed(dev, case, B, NT, FP8, h_sc=s)
    assert _same_bits(X8, X)
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(s[:, :ROWS], s_ref[:, :ROWS]) and bool((s[:, ROWS:] == 0x5A).all())


# ---------------------------------------------------------------------------- block_tail
COMBOS = [(u, h, tap) for u in (False, True) for h in (False, True) for tap in (False, True) if u or h or tap]


def _run_tail(dev, x, n_tok, *, u, aw, ln, post, h_dt, tap_dt, h_sc=None):
    """One block_tail call on fresh buffers; returns (X, H or None, tap or None)."""
    rows, width = x.shape
    X = _t(x, dev)
    H = tap = None
    if h_dt is not None:
        H = torch.empty(rows, width, device=dev, dtype=h_dt)
        if h_dt != FP8:
            H.fill_(float("nan"))
    if tap_dt is not None:
        tap = torch.full((rows // n_tok * (n_tok - 1), width), float("nan"), device=dev, dtype=tap_dt)
    ops.block_tail(X, n_tok, u=None if u is None else _t(u, dev), adapt_weight=aw,
                   ln=_dev_pair(ln, dev) if H is not None else None, h=H,
                   post=_dev_pair(post, dev) if tap is not None else None, tap=tap, h_sc=h_sc)
    return X, H, tap


def _check_tail(dev, x, u, n_tok, aw, use_u, use_h, use_tap, what):
    rows, width = x.shape
    ln, post = _ln_pair(width, 3), _ln_pair(width, 4)
    kw = dict(u=u if use_u else None, aw=aw, ln=ln, post=post)
    X, H, tap = _run_tail(dev, x, n_tok, h_dt=torch.float32 if use_h else None,
                          tap_dt=torch.float32 if use_tap else None, **kw)
    if use_u:
        _within(X, RR.blend(x, u, aw), RR.blend_tol(x, u, aw), f"{what} x")
    else:
        assert _same_bits(X, _t(x, dev)), f"{what}: x changed without an adapter"
    x_out = RR.f64(X)
    if use_h:
        ref = RR.layer_norm(x_out, *ln)
        _within(H, ref, RR.ln_tol(x_out, ln[0], ref), f"{what} h")
    if use_tap:
        src, dst = RR.tap_rows(rows, n_tok)
        assert tap.shape[0] == len(src) and sorted(dst) == list(range(tap.shape[0]))
        ref = RR.layer_norm(x_out[src], *post)
        _within(tap[torch.from_numpy(dst).to(dev)], ref, RR.ln_tol(x_out[src], post[0], ref), f"{what} tap")
    if use_h or use_tap:
        for dt in DT16:
            X16, H16, tap16 = _run_tail(dev, x, n_tok, h_dt=dt if use_h else None, tap_dt=dt if use_tap else None, **kw)
            assert _same_bits(X16, X)
            assert not use_h or _same_bits(H16, H.to(dt)), f"{what} h {dt}"
            assert not use_tap or _same_bits(tap16, tap.to(dt)), f"{what} tap {dt}"


@pytest.mark.parametrize("use_u,use_h,use_tap", COMBOS)
@pytest.mark.parametrize("width", WIDTHS)
def test_block_tail_combinations(dev, width, use_u, use_h, use_tap):
    """Every combination of adapter blend / next ln_1 / level tap at 3 images of 5 tokens; with the
    blend, at adapter weights 0.1 and 0 and norm ratios |x| / |u| from 1e-3 to 1e3."""
    x, u = RR.blend_inputs(ROWS, width)
    for aw in ((0.1, 0.0) if use_u else (0.0,)):
        _check_tail(dev, x, u, NT, aw, use_u, use_h, use_tap, f"block_tail {width} u={use_u} h={use_h} tap={use_tap} aw={aw}")


@pytest.mark.parametrize("batch,n_tok,width,use_h,use_tap", [(2, 577, 1024, True, True), (3, 77, 768, True, False)])
def test_block_tail_product_layouts(dev, batch, n_tok, width, use_h, use_tap):
    """The image engine's call (u + h + tap, 577 tokens at 1024) and the text engine's (u + h, 77 at 768)."""
    x, u = RR.blend_inputs(batch * n_tok, width)
    _check_tail(dev, x, u, n_tok, 0.1, True, use_h, use_tap, f"block_tail {batch}x{n_tok}x{width}")


@pytest.mark.parametrize("width", WIDTHS)
def test_block_tail_single_token_rows(dev, width):
    x, u = RR.blend_inputs(ROWS, width)
    _check_tail(dev, x, u, 1, 0.0, False, True, False, f"block_tail n_tok=1 {width}")


def test_block_tail_fp8_h_keeps_a_bf16_tap(dev):
    width = 768
    x, u = RR.blend_inputs(ROWS, width)
    kw = dict(u=u, aw=0.1, ln=_ln_pair(width, 3), post=_ln_pair(width, 4))
    _, H, tap = _run_tail(dev, x, NT, h_dt=torch.bfloat16, tap_dt=torch.bfloat16, **kw)
    _, H32, _ = _run_tail(dev, x, NT, h_dt=torch.float32, tap_dt=None, **kw)
    s = ops.mx_scales(ROWS, width, dev)
    _, q, tap8 = _run_tail(dev, x, NT, h_dt=FP8, tap_dt=torch.bfloat16, h_sc=s, **kw)
    assert q.dtype == FP8 and tap8.dtype == torch.bfloat16 and _same_bits(tap8, tap)
    q_ref, s_ref = torch.empty_like(q), ops.mx_scales(ROWS, width, dev)
    ops.quant_fp8_mx(H32, q_ref, s_ref)
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)) and torch.equal(s[:, :ROWS], s_ref[:, :ROWS])


# ---------------------------------------------------------------------------- text_embed_ln
@pytest.mark.parametrize("n,ctx", [(3, 77), (5, 7)])
@pytest.mark.parametrize("width", WIDTHS)
def test_text_embed_ln(dev, width, n, ctx):
    """x = tok_emb[tokens] + pos[t] bit for bit (one add has no ordering freedom), h = ln_1(x)."""
    rng = np.random.default_rng(31 * ctx + width)
    vocab = 50
    emb = rng.standard_normal((vocab, width)).astype(np.float32)
    pos = (rng.standard_normal((77, width)) * (1 + np.arange(77) % 5)[:, None]).astype(np.float32)
    tok = rng.integers(0, vocab, (n, ctx)).astype(np.int32)
    tok[0, 0], tok[-1, -1], tok[1, 2] = 0, vocab - 1, vocab - 1
    ln1 = _ln_pair(width, 5)
    tokens = _t(tok, dev)
    embd, posd, ln1d = _t(emb, dev), _t(pos, dev), _dev_pair(ln1, dev)
    X = torch.full((n * ctx, width), float("nan"), device=dev)
    H = torch.full((n * ctx, width), float("nan"), device=dev)
    ops.text_embed_ln(tokens, embd, posd, ln1d, X, H)
    x_ref = torch.from_numpy(emb)[torch.from_numpy(tok).long()] + torch.from_numpy(pos)[:ctx]
    assert _same_bits(X.cpu(), x_ref.reshape(n * ctx, width))
    x_out = RR.f64(X)
    ref = RR.layer_norm(x_out, *ln1)
    _within(H, ref, RR.ln_tol(x_out, ln1[0], ref), f"text_embed_ln h {n}x{ctx}x{width}")
    for dt in DT16:
        X16 = torch.empty_like(X)
        H16 = torch.empty(n * ctx, width, device=dev, dtype=dt)
        ops.text_embed_ln(tokens, embd, posd, ln1d, X16, H16)
        assert _same_bits(X16, X) and _same_bits(H16, H.to(dt)), dt


# ---------------------------------------------------------------------------- eot_ln
def _eot_rows(ctx):
    """Token rows whose maximum sits at 0, 63, 64 and ctx - 1, ties across lanes and inside one
    lane's stride (the smaller index wins), and a row of equal tokens."""
    eot = 49407
    spots = [(0,), (ctx - 1,)]
    if ctx > 70:
        spots += [(63,), (64,), (3, 70), (6, 70)]  # 3 / 70: lanes 3 and 6; 6 / 70: both lane 6
    else:
        spots += [(2, 5), (1, ctx - 1)]
    if ctx > 128:
        spots += [(65, 129), (1, 129)]             # lane 1 twice; lane 1's first and third element
    rows = []
    for k, s in enumerate(spots):
        r = (np.arange(ctx, dtype=np.int32) * 7 + k) % 40 + 1
        r[list(s)] = eot
        rows.append(r)
    rows.append(np.full(ctx, 5, dtype=np.int32))
    return np.stack(rows)


@pytest.mark.parametrize("ctx", [7, 77, 130])
@pytest.mark.parametrize("width", WIDTHS)
def test_eot_ln(dev, width, ctx):
    """n_seq = 5 sequences per call (the special rows in overlapping groups of five): the output is
    the LayerNorm of the row rows_ref.eot_index picks -- the same bits as ops.layernorm of those
    rows, and within ln_tol of float64."""
    n_seq = 5
    all_tok = _eot_rows(ctx)
    ln = _ln_pair(width, 6)
    lnd = _dev_pair(ln, dev)
    rng = np.random.default_rng(ctx + width)
    for g0 in range(0, len(all_tok) - n_seq + 1, 2):
        tok = all_tok[g0:g0 + n_seq]
        x = (rng.standard_normal((n_seq * ctx, width)) * (1 + np.arange(n_seq * ctx) % 11)[:, None]).astype(np.float32)
        xd = _t(x, dev)
        y = torch.full((n_seq, width), float("nan"), device=dev)
        ops.eot_ln(xd, _t(tok, dev), lnd, y)
        idx = RR.eot_index(tok)
        assert np.all(tok[np.arange(n_seq), idx] == tok.max(-1)) and np.all(idx <= ctx - 1)
        pick = np.arange(n_seq) * ctx + idx
        xs = np.ascontiguousarray(x[pick])
        y_ln = torch.empty(n_seq, width, device=dev)
        ops.layernorm(_t(xs, dev), lnd[0], lnd[1], y_ln)
        assert _same_bits(y, y_ln), f"eot_ln ctx {ctx} rows {g0}..: not the rows {list(idx)}"
        ref = RR.layer_norm(xs, *ln)
        _within(y, ref, RR.ln_tol(xs, ln[0], ref), f"eot_ln {ctx}x{width} group {g0}")
    assert g0 + n_seq == len(all_tok)  # every special row ran


# ---------------------------------------------------------------------------- l2_normalize
@pytest.mark.parametrize("dout", DT3)
@pytest.mark.parametrize("din", DT3)
@pytest.mark.parametrize("width", WIDTHS)
def test_l2_normalize(dev, width, din, dout):
    """x is a column view at the engines' segbuf offset (buf[:, 4 * 768:]); one all-zero row (exactly
    zero out, not NaN) and one row at scale 1e-10; a separate y for every dtype pair and in place
    when the dtypes agree."""
    rng = np.random.default_rng(width)
    x = rng.standard_normal((ROWS, width))
    x[13] *= 1e-10
    x[14] = 0.0
    off = 4 * 768
    buf = torch.full((ROWS, off + width), SENTINEL, device=dev, dtype=din)
    xv = buf[:, off:]
    xv.copy_(_t(x.astype(np.float32), dev))
    assert xv.data_ptr() % 16 == 0 and not xv.is_contiguous()
    ref = RR.l2_normalize(xv)  # float64 of the rounded input
    y32 = torch.full((ROWS, width), float("nan"), device=dev)
    ops.l2_normalize(xv, y32)
    _within(y32, ref, RR.l2_tol(ref), f"l2_normalize {din} {width}")
    assert bool((y32[14] == 0).all())
    y = torch.full((ROWS, width), float("nan"), device=dev, dtype=dout)
    ops.l2_normalize(xv, y)
    assert _same_bits(y, y32.to(dout))
    if din == dout:
        ops.l2_normalize(xv, xv)
        assert _same_bits(xv, y)
        assert _same_bits(buf[:, :off], torch.full((ROWS, off), SENTINEL, device=dev, dtype=din))


# ---------------------------------------------------------------------------- anchor_reduce
@pytest.mark.parametrize("dim", [100, 520, 768, 1024])
@pytest.mark.parametrize("n", [1, 2, 5, 35, 256])
def test_anchor_reduce(dev, n, dim):
    """normalize(mean_s normalize(emb_s)) into one column of T [dim, 2], the other column untouched:
    correlated prompts, independent rows, and correlated rows of scales 1e-2 .. 1e2 (where a dropped
    per-row normalisation is wrong by over 100 times the 5e-7 bound)."""
    rng = np.random.default_rng(1000 * n + dim)
    base = rng.standard_normal(dim)
    kinds = {"correlated": base + 0.1 * rng.standard_normal((n, dim)),
             "independent": rng.standard_normal((n, dim)),
             "scaled": (base + 0.1 * rng.standard_normal((n, dim))) * np.logspace(-2, 2, n)[:, None]}
    for name, e in kinds.items():
        e = e.astype(np.float32)
        for col in (0, 1):
            T = torch.full((dim, 2), SENTINEL, device=dev)
            ops.anchor_reduce(_t(e, dev), T, col)
            ref = RR.anchor_reduce(e)
            _within(T[:, col], ref, np.full(dim, RR.ANCHOR_ATOL), f"anchor_reduce {name} n={n} dim={dim} col={col}")
            assert _same_bits(T[:, 1 - col], torch.full((dim,), SENTINEL, device=dev))


# ---------------------------------------------------------------------------- im2col
@pytest.mark.parametrize("P,S,kp,batch", [(7, 28, 152, 3), (16, 1040, 768, 1), (16, 1024, 768, 1)])
@pytest.mark.parametrize("dt", DT3)
def test_im2col_fallback_exact(dev, P, S, kp, batch, dt):
    """The assertions of test_im2col_exact where aaclip_im2col takes im2col_kernel instead of the band
    kernel: an odd patch (7) and a band over 64 KiB (16 x 1040 x 4 = 66 560 B); 16 x 1024 is the
    largest band (65 536 B) that still takes the band kernel."""
    torch.manual_seed(S + P)
    C = 3
    base = torch.randn(batch * C * S * S + 1, device=dev)
    for img in (base[:-1].view(batch, C, S, S), base[1:].view(batch, C, S, S)):
        g = S // P
        cols = torch.full((batch * g * g, kp), float("nan"), device=dev, dtype=dt)
        ops.im2col(img, cols, P)
        ref = torch.nn.functional.unfold(img, P, stride=P).transpose(1, 2).reshape(batch * g * g, C * P * P)
        torch.cuda.synchronize()
        assert torch.equal(cols[:, :C * P * P], ref.to(dt))
        assert torch.equal(cols[:, C * P * P:], torch.zeros_like(cols[:, C * P * P:]))


# ---------------------------------------------------------------------------- wrapper rejections
def _colview(rows, width, dev, dt=torch.float32):
    """[rows, width] with a row stride of 2 * width: what a fused row kernel would misread."""
    return torch.zeros(rows, 2 * width, device=dev, dtype=dt)[:, :width]


def _as(t, dt):
    """t's shape in another dtype, inside an allocation at least as large as an fp32 one."""
    return torch.zeros((2 * t.shape[0],) + tuple(t.shape[1:]), device=t.device, dtype=dt)[:t.shape[0]]


def _rejects(call, **bad):
    """call(**good) with one operand replaced must raise before any launch."""
    with pytest.raises((ValueError, TypeError)):
        call(**bad)


def test_wrappers_reject_bad_operands_without_a_launch(dev):
    W_ = 768
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)  # noqa: E731
    vec, long_vec = z(W_), z(2 * W_)
    pair, bad_pairs = (vec, vec), [(long_vec, vec), (vec, long_vec), (_as(vec, torch.float16), vec), (vec, _as(vec, torch.float64))]
    tok = z(3, 7, dt=torch.int32)
    bad_toks = [z(3, 7, dt=torch.int64), z(3, 14, dt=torch.int32)[:, ::2], z(3, 14, dt=torch.int32)[:, :7]]
    rows = z(ROWS, W_)
    bad_rows = [_colview(ROWS, W_, dev), _as(rows, torch.bfloat16), _as(rows, torch.float64)]

    def embed(x=rows, cls=vec, pos=z(NT, W_), pre=pair, ln1=pair, h=z(ROWS, W_)):
        ops.embed_ln(x, cls, pos, pre, ln1, h, B, NT)

    for x in bad_rows:
        _rejects(embed, x=x)
    _rejects(embed, h=_colview(ROWS, W_, dev))
    _rejects(embed, h=_as(rows, torch.float64))
    for c in (long_vec, _as(vec, torch.float16)):
        _rejects(embed, cls=c)
    for p in (z(NT + 1, W_), _as(z(NT, W_), torch.float16), _colview(NT, W_, dev)):
        _rejects(embed, pos=p)
    for bp in bad_pairs:
        _rejects(embed, pre=bp)
        _rejects(embed, ln1=bp)

    def tail(x=rows, u=z(ROWS, W_), ln=pair, h=z(ROWS, W_), post=pair, tap=z(B * (NT - 1), W_), n_tok=NT):
        ops.block_tail(x, n_tok, u=u, adapt_weight=0.1, ln=ln, h=h, post=post, tap=tap)

    for x in bad_rows:
        _rejects(tail, x=x)
        _rejects(tail, u=x)
    _rejects(tail, h=_colview(ROWS, W_, dev))
    _rejects(tail, tap=_colview(B * (NT - 1), W_, dev))
    _rejects(tail, tap=z(ROWS, W_))
    _rejects(tail, n_tok=4)       # 15 rows are no whole number of 4-token images
    _rejects(tail, ln=None)       # h without its LayerNorm
    _rejects(tail, post=None)     # tap without ln_post
    for bp in bad_pairs:
        _rejects(tail, ln=bp)
        _rejects(tail, post=bp)

    def ln(x=rows, w=vec, b=vec, y=z(ROWS, W_)):
        ops.layernorm(x, w, b, y)

    for v in (long_vec, z(1024), _as(vec, torch.float16)):
        _rejects(ln, w=v)
        _rejects(ln, b=v)
    _rejects(ln, x=_as(rows, torch.bfloat16))

    def text(tokens=tok, emb=z(50, W_), pos=z(77, W_), ln1=pair, x=z(21, W_), h=z(21, W_)):
        ops.text_embed_ln(tokens, emb, pos, ln1, x, h)

    def eot(x=z(21, W_), tokens=tok, ln=pair, y=z(3, W_)):
        ops.eot_ln(x, tokens, ln, y)

    for t in bad_toks:
        _rejects(text, tokens=t)
        _rejects(eot, tokens=t)
    for x in (_colview(21, W_, dev), _as(z(21, W_), torch.bfloat16), z(22, W_)):
        _rejects(text, x=x)
        _rejects(eot, x=x)
    _rejects(text, h=_colview(21, W_, dev))
    _rejects(eot, y=_colview(3, W_, dev))
    _rejects(text, emb=_as(z(50, W_), torch.float16))
    _rejects(text, pos=z(6, W_))  # fewer positions than ctx
    _rejects(text, pos=_as(z(77, W_), torch.float16))
    for bp in bad_pairs:
        _rejects(text, ln1=bp)
        _rejects(eot, ln=bp)

    def anchor(emb=z(6, W_), T=z(W_, 2), col=0):
        ops.anchor_reduce(emb, T, col)

    for T in (z(W_, 4)[:, :2], _as(z(W_, 2), torch.float64), z(W_ + 1, 2), z(2 * W_)):
        _rejects(anchor, T=T)
    _rejects(anchor, col=2)
    _rejects(anchor, col=-1)
    _rejects(anchor, emb=_colview(6, W_, dev))
    _rejects(anchor, emb=z(257, W_))

    def l2(x=rows, y=z(ROWS, W_)):
        ops.l2_normalize(x, y)

    _rejects(l2, x=z(ROWS, 2 * W_)[:, ::2])
    _rejects(l2, y=z(ROWS, W_ + 2)[:, :W_])     # row stride no multiple of 4
    _rejects(l2, x=_as(rows, torch.float64))
    _rejects(l2, y=z(ROWS + 1, W_))
