"""Host-side checks of the forward row kernels (no GPU): tests/rows_ref.py, the float64 restatement
the GPU tests compare with, agrees with torch's float64 operators, with the float32 numpy oracle and
with the golden LayerNorm vectors; its error bounds leave a float32 implementation a factor of two;
its EOT rule is first-occurrence; and the eight C entry points reject bad arguments without a
launch."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aaclip import _lib
from oracle import aaclip_np, synth

import rows_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (768, 1024)


# ---------------------------------------------------------------------------- the references
@pytest.mark.parametrize("width", WIDTHS)
def test_references_agree_with_torch_float64(width):
    x, w, b = RR.ln_inputs(width)
    xt, wt, bt = (torch.from_numpy(a).double() for a in (x, w, b))
    ref = F.layer_norm(xt, (width,), wt, bt, 1e-5).numpy()
    got = RR.layer_norm(x, w, b)
    assert got.dtype == np.float64 and np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    scaled = xt * torch.logspace(-10, 2, 15, dtype=torch.float64)[:, None]  # the zero row stays zero: eps applies
    ref = F.normalize(scaled, dim=-1).numpy()
    got = RR.l2_normalize(scaled)
    assert np.abs(got - ref).max() <= 1e-15 and np.all(got[14] == 0)
    e = torch.from_numpy(np.random.default_rng(width).standard_normal((7, width)))
    m = F.normalize(e, dim=-1).mean(0)
    assert np.abs(RR.anchor_reduce(e) - F.normalize(m, dim=0).numpy()).max() <= 1e-15


def test_references_agree_with_the_float32_oracle_and_the_golden_vectors(golden):
    o = golden["ops"]
    sd = {}
    synth._ln(sd, 111, "visual.ln_pre", 1024)  # the fixture's weights: every synth tensor is seeded by its name
    x, w, b = o["ln_x"], sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"]
    ref = RR.layer_norm(x, w, b)
    tol = RR.ln_tol(x, w, ref)
    assert np.all(np.abs(aaclip_np.layer_norm(x, w, b) - ref) <= tol)
    assert np.all(np.abs(o["ln_y"] - ref) <= tol)  # the real reference's own float32 output
    ref = RR.l2_normalize(x)
    assert np.all(np.abs(aaclip_np.l2_normalize(x) - ref) <= RR.l2_tol(ref))


def test_token_and_tap_row_mapping_by_hand():
    """B = 2, n_tok = 3 written out: rows 0 and 3 are the CLS rows."""
    D = 4
    x = np.arange(6 * D, dtype=np.float64).reshape(6, D)
    x[[0, 3]] = np.nan
    cls, pos = np.full(D, 100.0), np.array([[1000.0] * D, [2000.0] * D, [3000.0] * D])
    e = RR.embed_rows(x, cls, pos, 3)
    assert np.array_equal(e[0], cls + 1000) and np.array_equal(e[3], cls + 1000)
    assert np.array_equal(e[1], x[1] + 2000) and np.array_equal(e[2], x[2] + 3000)
    assert np.array_equal(e[4], x[4] + 2000) and np.array_equal(e[5], x[5] + 3000)
    src, dst = RR.tap_rows(6, 3)
    assert list(src) == [1, 2, 4, 5] and list(dst) == [0, 1, 2, 3]
    src, dst = RR.tap_rows(15, 5)
    assert len(src) == 12 and list(dst) == list(range(12)) and not set(src) & {0, 5, 10}


# ---------------------------------------------------------------------------- the bounds leave headroom
def _ln32_one_pass(x, w, b):
    x = x.astype(np.float32)
    mean = x.mean(-1, keepdims=True, dtype=np.float32)
    var = (x * x).mean(-1, keepdims=True, dtype=np.float32) - mean * mean
    return (x - mean) / np.sqrt(np.maximum(var, 0) + np.float32(1e-5)) * w + b


@pytest.mark.parametrize("width", WIDTHS)
def test_ln_tol_holds_for_torch_float32_with_a_factor_of_two(width):
    """torch's own float32 CPU F.layer_norm against the float64 reference, worst |error| / ln_tol per
    family (768 / 1024): normal 0.11 / 0.16, mean100 0.18 / 0.14, outlier 0.07 / 0.06,
    small 0.02 / 0.03, constant 0 / 0, zero 0 / 0. A float32 restatement of the kernel's own
    two-pass order measured 0.28 (normal), 0.23 (mean100) and about 0.3 (outlier) at 768. All are
    at most 0.5, so the GPU kernel (FMA contraction, another sum order) keeps a factor of two. The
    same bound refuses a one-pass variance (mean100: over 1e3 times the bound), an unbiased variance
    and eps 1e-6."""
    x, w, b = RR.ln_inputs(width)
    ref = RR.layer_norm(x, w, b)
    tol = RR.ln_tol(x, w, ref)
    y = F.layer_norm(torch.from_numpy(x), (width,), torch.from_numpy(w), torch.from_numpy(b), 1e-5).numpy()
    ratio = np.abs(y.astype(np.float64) - ref) / tol
    for fam in RR.LN_FAMILIES:
        print(f"width {width} {fam}: worst |float32 - float64| / ln_tol = {ratio[RR.LN_FAMILY_ROWS[fam]].max():.3f}")
        assert ratio[RR.LN_FAMILY_ROWS[fam]].max() <= 0.5, fam
    # what the bound must refuse
    x64 = x.astype(np.float64)
    mean = x64.mean(-1, keepdims=True)
    d = x64 - mean
    var = (d * d).mean(-1, keepdims=True)
    unbiased = d / np.sqrt(var * width / (width - 1) + 1e-5) * w + b
    eps6 = d / np.sqrt(var + 1e-6) * w + b
    rows = RR.LN_FAMILY_ROWS
    assert (np.abs(unbiased - ref) / tol)[rows["normal"]].max() > 100
    assert (np.abs(eps6 - ref) / tol)[rows["small"]].max() > 100
    assert (np.abs(_ln32_one_pass(x, w, b) - ref) / tol)[rows["mean100"]].max() > 100


@pytest.mark.parametrize("aw", [0.1, 0.0])
@pytest.mark.parametrize("width", WIDTHS)
def test_blend_tol_holds_for_a_float32_restatement_with_a_factor_of_two(width, aw):
    """The kernel's blend restated in float32 numpy (aw (u xn / un) + (1 - aw) x, both norms float32)
    against the float64 reference: worst |error| / blend_tol 0.36 (768) and 0.38 (1024) at aw = 0.1 and 0 at
    aw = 0, inside the half the GPU kernel is left."""
    x, u = RR.blend_inputs(15, width)
    xn = np.sqrt((x * x).sum(-1, keepdims=True, dtype=np.float32))
    un = np.sqrt((u * u).sum(-1, keepdims=True, dtype=np.float32))
    a32 = np.float32(aw)
    y = a32 * (u * xn / un) + (np.float32(1) - a32) * x
    assert y.dtype == np.float32
    ratio = np.abs(y.astype(np.float64) - RR.blend(x, u, aw)) / RR.blend_tol(x, u, aw)
    print(f"width {width} aw {aw}: worst |float32 - float64| / blend_tol = {ratio.max():.3f}")
    assert ratio.max() <= 0.5
    r = np.linalg.norm(x.astype(np.float64), axis=1) / np.linalg.norm(u.astype(np.float64), axis=1)
    assert r.min() < 2e-3 and r.max() > 5e2


def test_l2_and_anchor_bounds_hold_for_float32_restatements():
    """float32 numpy restatements against float64: l2_normalize worst |error| / l2_tol 0.29;
    anchor_reduce worst absolute error 8e-8 against the 5e-7 bound, while dropping the per-row
    normalisation is wrong by several 1e-3 (over 100 times the bound) on rows of unequal scale."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((15, 768)) * np.logspace(-10, 2, 15)[:, None]).astype(np.float32)
    inv = np.float32(1) / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True, dtype=np.float32)), np.float32(1e-12))
    ref = RR.l2_normalize(x)
    ratio = np.abs((x * inv).astype(np.float64) - ref) / RR.l2_tol(ref)
    print(f"l2_normalize: worst ratio {ratio.max():.3f}")
    assert ratio.max() <= 0.5
    worst = 0.0
    for n in (1, 2, 5, 35, 256):
        for dim in (100, 520, 768, 1024):
            base = rng.standard_normal(dim)
            e = ((base + 0.1 * rng.standard_normal((n, dim))) * np.logspace(-2, 2, n)[:, None]).astype(np.float32)
            en = e / np.sqrt((e * e).sum(-1, keepdims=True, dtype=np.float32))
            m = en.sum(0, dtype=np.float32) / np.float32(n)
            t = m / np.sqrt((m * m).sum(dtype=np.float32))
            worst = max(worst, np.abs(t.astype(np.float64) - RR.anchor_reduce(e)).max())
            if n >= 5:
                m = e.astype(np.float64).mean(0)
                assert np.abs(m / np.linalg.norm(m) - RR.anchor_reduce(e)).max() > 100 * RR.ANCHOR_ATOL
    print(f"anchor_reduce: worst absolute error {worst:.2e}")
    assert worst <= 0.5 * RR.ANCHOR_ATOL


# ---------------------------------------------------------------------------- EOT tie rule
def test_eot_index_returns_the_first_occurrence():
    ctx, eot = 77, 49407
    rows = []
    for pos in ((3, 70), (6, 70), (0,), (63,), (64,), (ctx - 1,)):  # across lanes; inside lane 6's stride; edges
        r = np.arange(1, ctx + 1, dtype=np.int32) % 40 + 1
        r[list(pos)] = eot
        rows.append(r)
    rows.append(np.full(ctx, 5, dtype=np.int32))  # all equal
    tok = np.stack(rows)
    assert list(RR.eot_index(tok)) == [3, 6, 0, 63, 64, ctx - 1, 0]
    assert list(RR.eot_index(torch.from_numpy(tok))) == [3, 6, 0, 63, 64, ctx - 1, 0]


# ---------------------------------------------------------------------------- C ABI
P, Q, R_, W, S5, S6, S7, S8 = (ctypes.c_void_p(a << 20) for a in range(1, 9))
F32, BF16, FP8 = _lib.F32, _lib.BF16, _lib.FP8


def _bad(fn, good):
    """Call fn with one or more of the well-formed arguments replaced (`good` itself never runs)."""
    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    return bad


def _nulls(bad, idx):
    return all(bad(**{f"a{i}": None}) == 1 for i in idx)


def test_embed_ln_and_block_tail_reject_bad_arguments_without_a_launch():
    lib = _lib.lib()
    # (out_dtype, x, cls, pos, ln_pre w b, ln1 w b, h, batch, n_tok, width, h_mx, ld_mx, stream)
    bad = _bad(lib.aaclip_embed_ln, [F32, P, Q, R_, W, S5, S6, S7, S8, 3, 5, 768, None, 0, None])
    assert _nulls(bad, range(1, 9))
    assert bad(a11=512) == 1 and bad(a11=0) == 1 and bad(a11=1280) == 1
    assert bad(a10=1) == 1 and bad(a10=0) == 1 and bad(a9=0) == 1
    assert bad(a0=FP8) == 1 and bad(a0=FP8, a12=P, a13=14) == 1 and bad(a0=7) == 1  # no scales; ld_mx < 15 rows
    # (out_dtype, x, u, aw, ln w b, h, post w b, tap, rows, n_tok, width, h_mx, ld_mx, stream)
    bad = _bad(lib.aaclip_block_tail, [F32, P, Q, 0.1, R_, W, S5, S6, S7, S8, 15, 5, 768, None, 0, None])
    assert bad(a1=None) == 1 and bad(a12=512) == 1 and bad(a12=1280) == 1
    assert bad(a10=0) == 1 and bad(a11=0) == 1
    assert bad(a10=16) == 1 and bad(a11=1) == 1                   # tap: rows % n_tok, no patch rows
    assert bad(a7=None) == 1 and bad(a8=None) == 1                # tap without post
    assert bad(a4=None) == 1 and bad(a5=None) == 1                # h without ln
    assert bad(a0=FP8) == 1 and bad(a0=FP8, a13=P, a14=14) == 1 and bad(a0=7) == 1


def test_layernorm_and_l2_normalize_reject_bad_arguments_without_a_launch():
    lib = _lib.lib()
    # (out_dtype, x, ldx, w, b, y, ldy, rows, width, y_mx, ld_mx, stream)
    bad = _bad(lib.aaclip_layernorm, [F32, P, 768, Q, R_, W, 768, 15, 768, None, 0, None])
    assert _nulls(bad, (1, 3, 4, 5))
    assert bad(a8=512) == 1 and bad(a7=-1) == 1
    assert bad(a2=764) == 1 and bad(a2=770) == 1 and bad(a6=764) == 1 and bad(a6=770) == 1
    assert bad(a0=FP8) == 1 and bad(a0=FP8, a9=S5, a10=14) == 1 and bad(a0=7) == 1
    assert bad(a0=FP8, a9=S5, a10=16, a6=772) == 1                # fp8 rows are packed: ldy == width
    assert bad(a7=0) == 0                                         # nothing to do is not an error
    # (in_dtype, out_dtype, x, ldx, y, ldy, rows, width, stream)
    bad = _bad(lib.aaclip_l2_normalize, [F32, BF16, P, 768, Q, 768, 15, 768, None])
    assert _nulls(bad, (2, 4))
    assert bad(a0=FP8) == 1 and bad(a1=FP8) == 1 and bad(a0=7) == 1
    assert bad(a3=764) == 1 and bad(a3=770) == 1 and bad(a5=764) == 1 and bad(a5=770) == 1
    assert bad(a7=512) == 1 and bad(a6=-1) == 1
    assert bad(a6=0) == 0


def test_text_rows_anchor_and_im2col_reject_bad_arguments_without_a_launch():
    lib = _lib.lib()
    # (out_dtype, tokens, tok_emb, pos, ln1 w b, x, h, n_seq, ctx, width, stream)
    bad = _bad(lib.aaclip_text_embed_ln, [F32, P, Q, R_, W, S5, S6, S7, 3, 7, 768, None])
    assert _nulls(bad, range(1, 8))
    assert bad(a0=FP8) == 1 and bad(a0=7) == 1 and bad(a8=0) == 1 and bad(a9=0) == 1 and bad(a10=512) == 1
    # (out_dtype, x, tokens, w, b, y, n_seq, ctx, width, stream)
    bad = _bad(lib.aaclip_eot_ln, [F32, P, Q, R_, W, S5, 3, 7, 768, None])
    assert _nulls(bad, range(1, 6))
    assert bad(a0=FP8) == 1 and bad(a0=7) == 1 and bad(a6=0) == 1 and bad(a7=0) == 1 and bad(a8=512) == 1
    # (emb, n, dim, T, col, ncols, stream)
    bad = _bad(lib.aaclip_anchor_reduce, [P, 6, 768, Q, 0, 2, None])
    assert _nulls(bad, (0, 3))
    assert bad(a1=0) == 1 and bad(a1=257) == 1 and bad(a2=1025) == 1 and bad(a2=0) == 1
    assert bad(a4=2) == 1 and bad(a4=-1) == 1
    # (out_dtype, img, cols, batch, channels, img_size, patch, k_padded, stream)
    bad = _bad(lib.aaclip_im2col, [F32, P, Q, 1, 3, 28, 14, 640, None])
    assert _nulls(bad, (1, 2))
    assert bad(a0=FP8) == 1 and bad(a3=0) == 1 and bad(a4=0) == 1 and bad(a6=0) == 1
    assert bad(a5=30) == 1 and bad(a7=644) == 1 and bad(a7=584) == 1   # S % P; kp % 8; kp < 3 * 14 * 14
