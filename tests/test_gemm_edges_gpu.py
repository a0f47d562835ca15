"""aaclip_gemm and aaclip_gemm_scores (aa-clip_amd/csrc/gemm.hip) at their tile edges, on strided
operands inside guarded buffers, against the float64 reference and the per-element bound of
tests/gemm_ref.py (checked on the host in tests/test_gemm_host.py).

Every operand is a view inside a larger buffer: A and W with a leading dimension of K + 64 and three
guard rows above and below, all of it NaN outside the view, so a read past row M - 1, past row N - 1 of
W or past column K - 1 poisons the output; C, the aux copy and the score partials with a leading
dimension of N + 64 (N / 8 + 8 for the partials) and guard rows, pre-filled with a sentinel that must
survive bit for bit wherever the kernel has no business writing (the aux copy at N + 192, so that no two
of ldc, ldr and ldaux agree); the residual with its own leading dimension N + 128 and NaN padding; the
bias between NaN pads. Each case also runs on contiguous, exactly sized operands and must give the same
bits, and every forced tile family must give the bits of the 64x64 family (aaclip_gemm_pin: "a pin
changes speed, never bits").

Shapes per family (tile BM x BN): M in {1, 17, BM - 1, BM + 1, 4 BM + 1} crossed with K in
{64, 128, 192, 320} (1, 2, 3, 5 K-steps) at N = BN (128 for the 64x64 family: the entry takes
N % 128 == 0 only), then the other N at (BM + 1, 128); the epilogues rotate over the cases. The fp32
kernel: the same with its 64x64 tile and K in {16, 32, 48, 80}.

Measured on the MI355X (profiles/r13/gemm_edge_error_ratios.txt): worst error / bound into an fp32 C
0.031 (16-bit kernels; 0.64 with erf GELU, where gelu_fast's form error is most of the bound), 0.17
(fp32 kernel), 0.010 (score partials); into a 16-bit C up to 0.999, the rounding of the output itself.
The file takes 11 s, most of it the float64 references."""
import functools

import numpy as np
import pytest
import torch

from aaclip import _lib, ops

import gemm_ref as GR

pytestmark = pytest.mark.gpu

SENTINEL = -7.25  # exact in every dtype used here
GUARD = 3
TILES = {1: (256, 256), 2: (256, 128), 3: (256, 256), 8: (320, 256), 9: (128, 128), 11: (64, 64)}
# N of the M x K cross: the family's BN, but 128 for the 64x64 family (aaclip_gemm takes N % 128 == 0
# only, so its tile always has a right-hand neighbour); then 2 BN and the smallest N off 256 it allows
MAIN_N = {1: 256, 2: 128, 3: 256, 8: 256, 9: 128, 11: 128, 0: 256}
OTHER_N = {1: (512,), 2: (256,), 3: (512,), 8: (512,), 9: (256,), 11: (256, 384), 0: (128, 512)}
FAMILIES = (0, 1, 2, 3, 8, 9, 11)
KINDS16 = ("bf16", "f16")
TDT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
K16 = (64, 128, 192, 320)
K32 = (16, 32, 48, 80)
# (epilogue, C dtype: "f32" or "h" = the operands' 16-bit type): the rotation over the cases
ROTATION = (("none", "f32"), ("bias", "h"), ("bias+gelu", "h"), ("bias+qgelu", "h"), ("leaky", "f32"),
            ("bias+resid", "f32"), ("bias+resid+aux", "f32"), ("leaky+resid", "h"),
            ("bias+gelu+resid+aux", "f32"), ("bias+aux", "h"), ("none", "h"), ("bias", "f32"),
            ("bias+gelu", "f32"), ("bias+qgelu", "f32"), ("leaky", "h"), ("bias+resid", "h"))


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded(data, rows, cols, dt, ld, fill, dev):
    """(buffer [rows + 2 GUARD, ld] filled with `fill`, its view [rows, cols]); `data` (numpy, or
    None) is copied into the view. The view's first element stays 16-byte aligned."""
    buf = torch.full((rows + 2 * GUARD, ld), fill, dtype=dt, device=dev)
    view = buf[GUARD:GUARD + rows, :cols]
    if data is not None:
        view.copy_(torch.from_numpy(np.array(data)).to(dev))
    assert view.data_ptr() % 16 == 0 and view.stride(0) == ld
    return buf, view


def _sentinels_intact(buf, written_rows, cols, what):
    """Everything of the guarded buffer outside view[written_rows, :cols] still holds the sentinel."""
    got = _bits(buf.cpu())
    keep = torch.ones(got.shape, dtype=torch.bool)
    keep[GUARD + torch.as_tensor(np.array(written_rows)), :cols] = False
    want = _bits(torch.tensor([SENTINEL], dtype=buf.dtype))[0]
    bad = (got != want) & keep
    assert not bad.any(), f"{what}: wrote outside its rows / columns, first at (row, col) {bad.nonzero()[0].tolist()} " \
                          f"of the guarded buffer (view starts at row {GUARD})"


class variant:
    """aaclip_set_gemm_variant for the duration of a block (process-global: always reset)."""

    def __init__(self, fam):
        self.fam = fam

    def __enter__(self):
        assert _lib.lib().aaclip_set_gemm_variant(self.fam) == 0

    def __exit__(self, *exc):
        _lib.lib().aaclip_set_gemm_variant(0)


@functools.lru_cache(maxsize=4)
def _case(kind, M, N, K, epi, out):
    """Inputs, float64 reference and bounds of one case (shared by the families and layouts)."""
    has_bias, act, has_res, has_aux, remap = GR.EPILOGUES[epi]
    rm = GR.REMAP if remap else None
    a, w, bias, resid = GR.gemm_inputs(M, N, K, kind, 0, rm)
    kw = dict(bias=bias if has_bias else None, act=act, residual=resid if has_res else None, row_remap=rm)
    ref, dst = GR.gemm_ref(a, w, **kw)
    in16 = kind != "f32"
    h = kind if in16 else "bf16"
    tol = GR.gemm_bound(a, w, in16=in16, out="f32" if out == "f32" else h, **kw)
    tol_aux = GR.gemm_bound(a, w, in16=in16, out=h, **kw) if has_aux else None
    for x in (a, w, bias, resid, ref, dst, tol):
        x.setflags(write=False)
    return a, w, kw, ref, dst, tol, tol_aux, h


def _launch(dev, kind, fam, M, N, K, epi, out, *, strided=True, alias=False, a_data=None):
    """One aaclip_gemm launch under tile family `fam`; returns (C rows in source order, aux rows or None)
    on the CPU. strided: guarded views, sentinel and NaN checks; else contiguous, exactly sized.
    alias: the residual is C itself (in place, as the engine's out-proj / c_proj call it)."""
    a, w, kw, ref, dst, tol, tol_aux, h = _case(kind, M, N, K, epi, out)
    has_bias, act, has_res, has_aux, remap = GR.EPILOGUES[epi]
    rows = GR.rows_out(M, kw["row_remap"])
    dt, cdt, hdt = TDT[kind], (torch.float32 if out == "f32" else TDT[h]), TDT[h]
    a = a if a_data is None else a_data
    nan = float("nan")
    if strided:
        _, ta = _guarded(a, M, K, dt, K + 64, nan, dev)
        _, tw = _guarded(w, N, K, dt, K + 64, nan, dev)
        cbuf, tc = _guarded(None, rows, N, cdt, N + 64, SENTINEL, dev)
        tr = _guarded(kw["residual"], rows, N, torch.float32, N + 128, nan, dev)[1] if has_res else None
        abuf, tx = _guarded(None, rows, N, hdt, N + 192, SENTINEL, dev) if has_aux else (None, None)
        tb = None
        if has_bias:
            bb = torch.full((N + 8,), nan, device=dev)
            tb = bb[4:4 + N]
            tb.copy_(torch.from_numpy(np.array(kw["bias"])).to(dev))
    else:
        t = lambda x, d: torch.from_numpy(np.array(x)).to(dev).to(d)
        ta, tw = t(a, dt), t(w, dt)
        tc = torch.full((rows, N), SENTINEL, dtype=cdt, device=dev)
        tr = t(kw["residual"], torch.float32) if has_res else None
        tx = torch.full((rows, N), SENTINEL, dtype=hdt, device=dev) if has_aux else None
        tb = t(kw["bias"], torch.float32) if has_bias else None
    if alias:
        assert has_res and cdt == torch.float32
        tc[dst.tolist()] = tr[dst.tolist()]
        tr = tc
    rg, rgo, roff = kw["row_remap"] or (0, 0, 0)
    gelu = "quick" if "qgelu" in act else "gelu" in act
    with variant(fam):
        ops.gemm(ta, tw, tc, bias=tb, gelu=gelu, leaky="leaky" in act, residual=tr, aux=tx, row_group=rg,
                 row_group_out=rgo, row_offset=roff)
    what = f"{kind} family {fam} M {M} N {N} K {K} {epi} -> {out}{' in place' if alias else ''}"
    if strided:
        _sentinels_intact(cbuf, dst, N, what + " C")
        if has_aux:
            _sentinels_intact(abuf, dst, N, what + " aux")
    else:
        skipped = sorted(set(range(rows)) - set(dst.tolist()))
        assert bool((tc[skipped] == SENTINEL).all()), what
    rows_of = lambda x: x.cpu()[dst.tolist()]
    return rows_of(tc), (rows_of(tx) if has_aux else None)


def _within(got, ref, tol, what, tag):
    err = np.abs(GR.f64(got) - ref)
    ok = err <= tol
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nanmax(np.where(err > 0, err / tol, 0.0)))
    print(f"RATIO {tag} | {what} | worst error / bound {ratio:.3f}")
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} elements outside the bound, first at {np.argwhere(~ok)[0]}, " \
                     f"worst error / bound {ratio:.3f}"


def _check(dev, kind, fam, M, N, K, epi, out, alias=False):
    """The per-case assertions: finite, inside the bound, aux = rounded C, strided = contiguous bits,
    forced family = family 11 bits (family 11 itself and the default dispatch: against each other)."""
    a, w, kw, ref, dst, tol, tol_aux, h = _case(kind, M, N, K, epi, out)
    what = f"{kind} family {fam} M {M} N {N} K {K} {epi} -> {out}{' in place' if alias else ''}"
    c, x = _launch(dev, kind, fam, M, N, K, epi, out, alias=alias)
    assert bool(torch.isfinite(c).all()), f"{what}: a NaN from the padding or the guard rows reached C"
    cls = "fp32" if kind == "f32" else ("8-phase" if fam == 3 and not (x is not None and out != "f32") else
                                        "16-bit generic")
    _within(c, ref, tol, what, f"{cls} | {epi} -> {out}")
    if x is not None:
        assert bool(torch.isfinite(x).all()), what
        _within(x, ref, tol_aux, what + " aux", f"{cls} | {epi} aux")
        assert _same_bits(x, c.to(x.dtype)), f"{what}: aux is not C rounded once"
    cc, xc = _launch(dev, kind, fam, M, N, K, epi, out, strided=False, alias=alias)
    assert _same_bits(c, cc), f"{what}: the strided result differs from the contiguous one"
    assert x is None or _same_bits(x, xc), f"{what}: the strided aux differs from the contiguous one"
    if kind != "f32":
        other = 0 if fam == 11 else 11
        co, xo = _launch(dev, kind, other, M, N, K, epi, out, alias=alias)
        assert _same_bits(c, co), f"{what}: bits differ from family {other}"
        assert x is None or _same_bits(x, xo), f"{what}: aux bits differ from family {other}"
    return c, x


def _cases(BM, N0, ks, other_n):
    i = 0
    for M in (1, 17, BM - 1, BM + 1, 4 * BM + 1):
        for K in ks:
            yield (M, N0, K) + ROTATION[i % len(ROTATION)]
            i += 1
    for N in other_n:
        yield (BM + 1, N, ks[1]) + ROTATION[i % len(ROTATION)]
        i += 1


# ---------------------------------------------------------------------------- the 16-bit families
@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("fam", FAMILIES)
def test_family_at_its_tile_edges(dev, fam, kind):
    BM = TILES.get(fam, (256, 256))[0]  # the default dispatch: the 256-row shapes
    cases = list(_cases(BM, MAIN_N[fam], K16, OTHER_N[fam]))
    assert {c[3:] for c in cases} >= set(ROTATION)
    for M, N, K, epi, out in cases:
        _check(dev, kind, fam, M, N, K, epi, out)


@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("fam", FAMILIES)
def test_residual_in_place(dev, fam, kind):
    """residual = C, the engine's out-proj / c_proj call: the bits of the out-of-place call."""
    BM, BN = TILES.get(fam, (256, 256))[0], MAIN_N[fam]
    for epi in ("bias+resid", "bias+resid+aux"):
        c, x = _check(dev, kind, fam, BM + 1, BN, 128, epi, "f32", alias=True)
        c2, x2 = _launch(dev, kind, fam, BM + 1, BN, 128, epi, "f32")
        assert _same_bits(c, c2) and (x is None or _same_bits(x, x2))


@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("fam", FAMILIES)
def test_row_remap_with_a_group_that_divides_no_tile(dev, fam, kind):
    """row_group 5 -> 7 at offset 2, M = 5 * 53: source rows land where gemm_ref says, the two skipped
    rows of every group keep the sentinel in C and in aux (checked in _launch for both layouts), and the
    residual is read from the remapped row at its own leading dimension."""
    BN = MAIN_N[fam]
    M = 5 * 53
    assert list(GR.remap_rows(M, GR.REMAP)[:6]) == [2, 3, 4, 5, 6, 9] and GR.rows_out(M, GR.REMAP) == 52 * 7 + 7
    for epi, out, K in (("remap", "f32", 64), ("remap+resid+aux", "f32", 192), ("remap", "h", 128)):
        _check(dev, kind, fam, M, BN, K, epi, out)


def _row_isolation(dev, kind, fam, BM, BN, K):
    M = BM + 1
    clean, _ = _launch(dev, kind, fam, M, BN, K, "bias", "f32")
    a = _case(kind, M, BN, K, "bias", "f32")[0].copy()
    a[M - 1, 5] = np.nan
    for strided in (True, False):
        got, _ = _launch(dev, kind, fam, M, BN, K, "bias", "f32", strided=strided, a_data=a)
        assert bool(torch.isnan(got[M - 1]).all()), "row M - 1 must be NaN in every column"
        assert _same_bits(got[:M - 1], clean[:M - 1]), "a NaN in row M - 1 of A changed another row"


@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("fam", FAMILIES)
def test_row_isolation(dev, fam, kind):
    """A NaN in the last valid row of A (row M - 1, alone in the ragged last tile) makes exactly that
    row of the output NaN; no other row changes a bit."""
    _row_isolation(dev, kind, fam, TILES.get(fam, (256, 256))[0], MAIN_N[fam], 128)


def test_row_isolation_fp32(dev):
    _row_isolation(dev, "f32", 0, 64, 64, 32)


# ---------------------------------------------------------------------------- the fp32 kernel
def test_fp32_kernel_at_its_tile_edges(dev):
    """64x64 tile, K-step 16: the M x K cross with every epilogue, fp32 and bf16 C, the bf16 aux copy
    beside an fp32 C, the second tile column, and M = 9 (below one 16-row MFMA group)."""
    cases = list(_cases(64, 64, K32, (128,))) + [(9, 64, 48, "bias+gelu+resid+aux", "f32"), (9, 128, 16, "leaky", "h")]
    assert {c[3:] for c in cases} >= set(ROTATION)
    for M, N, K, epi, out in cases:
        _check(dev, "f32", 0, M, N, K, epi, out)
    for epi, out, K in (("remap", "f32", 16), ("remap+resid+aux", "f32", 48), ("remap", "h", 32)):
        _check(dev, "f32", 0, 5 * 53, 64, K, epi, out)
    for epi in ("bias+resid", "bias+resid+aux"):
        c, x = _check(dev, "f32", 0, 65, 64, 32, epi, "f32", alias=True)
        c2, x2 = _launch(dev, "f32", 0, 65, 64, 32, epi, "f32")
        assert _same_bits(c, c2) and (x is None or _same_bits(x, x2))


# ---------------------------------------------------------------------------- the wrapper's own checks
def test_ops_gemm_rejects_a_16_bit_row_stride_off_16_bytes(dev):
    a = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(128, 64, dtype=torch.bfloat16, device=dev)
    out = torch.zeros(4, 132, dtype=torch.bfloat16, device=dev)[:, :128]
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.gemm(a, w, out)
    aux = torch.zeros(4, 132, dtype=torch.bfloat16, device=dev)[:, :128]
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.gemm(a, w, torch.zeros(4, 128, device=dev), aux=aux)
    ops.gemm(a, w, torch.zeros(4, 132, device=dev)[:, :128])  # an fp32 C keeps % 4


# ---------------------------------------------------------------------------- operands of 2 GiB and more
def _far_apart(rows, cols, ld, dt, dev):
    """A [rows, cols] view whose rows are ld elements apart, in a buffer that is allocated but never
    filled (only the view is written)."""
    try:
        buf = torch.empty((rows - 1) * ld + cols, dtype=dt, device=dev)
    except (torch.OutOfMemoryError, RuntimeError) as e:
        pytest.skip(f"cannot allocate {((rows - 1) * ld + cols) * 2 / 2 ** 30:.1f} GiB for the far-apart operand: {e}")
    return buf, buf.as_strided((rows, cols), (ld, 1))


@pytest.mark.parametrize("which", ["A", "W"])
def test_operands_of_2_gib_leave_the_8_phase_family(dev, which):
    """M * lda * 2 >= 2^31 (or N * ldw * 2): the 8-phase kernel's 32-bit buffer offsets cannot reach,
    so the dispatch must hand over to a kernel with 64-bit addressing, under the default dispatch, a
    forced family 3 and a forced family 8 alike: bits of the contiguous result, inside the bound."""
    M, N, K, kind = 257, 256, 64, "bf16"
    a, w, kw, ref, dst, tol, _, _ = _case(kind, M, N, K, "none", "f32")
    want, _ = _launch(dev, kind, 0, M, N, K, "none", "f32", strided=False)
    ta = torch.from_numpy(np.array(a)).to(dev).to(torch.bfloat16)
    tw = torch.from_numpy(np.array(w)).to(dev).to(torch.bfloat16)
    if which == "A":
        buf, far = _far_apart(M, K, 2 ** 22, torch.bfloat16, dev)
        far.copy_(ta)
        ta = far
        assert M * far.stride(0) * 2 >= 2 ** 31
    else:
        buf, far = _far_apart(N, K, 2 ** 23, torch.bfloat16, dev)
        far.copy_(tw)
        tw = far
        assert N * far.stride(0) * 2 >= 2 ** 31
    for fam in (0, 3, 8):
        cbuf, tc = _guarded(None, M, N, torch.float32, N + 64, SENTINEL, dev)
        with variant(fam):
            ops.gemm(ta, tw, tc)
        what = f"far-apart {which}, family {fam}"
        _sentinels_intact(cbuf, dst, N, what)
        got = tc.cpu()
        assert _same_bits(got, want), f"{what}: bits differ from the contiguous result"
        _within(got, ref, tol, what, "16-bit generic | none -> f32 (2 GiB operand)")
    if which == "A":  # aaclip_gemm_scores has a !fits branch of its own
        T = GR.anchors(64)
        want_p = _scores(dev, kind, 0, M, N, K, 64, 0, strided=False)
        got_p = _scores(dev, kind, 0, M, N, K, 64, 0, a_tensor=ta)
        assert _same_bits(got_p, want_p), "scores, far-apart A: bits differ from the contiguous result"
        v, _ = GR.gemm_ref(a, w)
        _within(got_p.reshape(M, N // 32, 4), GR.scores_ref(v, T, 64), _scores_tol(a, w, "none", T, 64),
                "scores, far-apart A", "scores | none (2 GiB operand)")
    del buf


# ---------------------------------------------------------------------------- aaclip_gemm_scores
def _scores_tol(a, w, act, T, tp):
    v, _ = GR.gemm_ref(a, w, act=act)
    tol = GR.scores_bound(v, GR.gemm_bound(a, w, act=act), T, tp)
    tol[..., 3] = 0.0
    return tol


def _scores(dev, kind, fam, M, N, K, tp, epi, *, strided=True, a_tensor=None):
    """One aaclip_gemm_scores launch through the C ABI (t_period is a free argument there); returns the
    partials [M, N / 8] on the CPU."""
    a, w, _, _ = GR.gemm_inputs(M, N, K, kind, 0)
    dt = TDT[kind]
    T = torch.from_numpy(GR.anchors(tp)).to(dev)
    nan = float("nan")
    if strided:
        ta = _guarded(a, M, K, dt, K + 64, nan, dev)[1]
        tw = _guarded(w, N, K, dt, K + 64, nan, dev)[1]
        pbuf, tp_ = _guarded(None, M, N // 8, torch.float32, N // 8 + 8, SENTINEL, dev)
    else:
        ta, tw = (torch.from_numpy(x).to(dev).to(dt) for x in (a, w))
        tp_ = torch.full((M, N // 8), SENTINEL, device=dev)
    if a_tensor is not None:
        ta = a_tensor
    with variant(fam):
        _lib.call("aaclip_gemm_scores", ops.dtag(ta), M, N, K, ops._ptr(ta), ta.stride(0), ops._ptr(tw), tw.stride(0),
                  epi, ops._ptr(T), tp, ops._ptr(tp_), tp_.stride(0), torch.cuda.current_stream().cuda_stream)
    if strided:
        _sentinels_intact(pbuf, np.arange(M), N // 8, f"scores {kind} family {fam} M {M} N {N} K {K}")
    return tp_.cpu()


@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("fam", FAMILIES)
def test_scores_at_the_tile_edges(dev, fam, kind):
    """part[m][g] = {sum v^2, sum v t0, sum v t1, 0} over 32 columns against the float64 reference and
    scores_bound; the fourth lane exactly 0; strided = contiguous bits; every family the bits of family
    11; and the partials of a row do not depend on M."""
    BM = TILES.get(fam, (256, 256))[0]
    i = 0
    for N, tp in ((256, 64), (512, 128)):
        for K in (64, 192):
            for M in (1, 17, BM - 1, BM + 1, 4 * BM + 1):
                epi, act = ((0, "none"), (_lib.EPI_LEAKY, "leaky"))[i % 2]  # 5 values of M: both at every (N, K)
                i += 1
                a, w, _, _ = GR.gemm_inputs(M, N, K, kind, 0)
                T = GR.anchors(tp)
                what = f"scores {kind} family {fam} M {M} N {N} K {K} t_period {tp} {act}"
                got = _scores(dev, kind, fam, M, N, K, tp, epi)
                assert bool(torch.isfinite(got).all()), what
                g4 = got.reshape(M, N // 32, 4)
                assert bool((_bits(g4[..., 3]) == 0).all()), f"{what}: the fourth lane is not +0.0"
                v, _ = GR.gemm_ref(a, w, act=act)
                _within(g4, GR.scores_ref(v, T, tp), _scores_tol(a, w, act, T, tp), what, f"scores | {act}")
                assert _same_bits(got, _scores(dev, kind, fam, M, N, K, tp, epi, strided=False)), what
                other = 0 if fam == 11 else 11
                assert _same_bits(got, _scores(dev, kind, other, M, N, K, tp, epi)), f"{what}: differs from {other}"


@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("fam", FAMILIES)
def test_scores_of_a_row_do_not_depend_on_the_batch(dev, fam, kind):
    """The first 17 rows of M = BM + 1 are the rows of M = 17, bit for bit (same A rows, same W)."""
    BM = TILES.get(fam, (256, 256))[0]
    N, K, tp = 256, 192, 64
    a_big, w, _, _ = GR.gemm_inputs(BM + 1, N, K, kind, 0)
    T = torch.from_numpy(GR.anchors(tp)).to(dev)
    tw = _guarded(w, N, K, TDT[kind], K + 64, float("nan"), dev)[1]
    res = []
    for M in (BM + 1, 17):
        ta = _guarded(a_big[:M], M, K, TDT[kind], K + 64, float("nan"), dev)[1]
        pbuf, part = _guarded(None, M, N // 8, torch.float32, N // 8 + 8, SENTINEL, dev)
        with variant(fam):
            _lib.call("aaclip_gemm_scores", ops.dtag(ta), M, N, K, ops._ptr(ta), ta.stride(0), ops._ptr(tw),
                      tw.stride(0), _lib.EPI_LEAKY, ops._ptr(T), tp, ops._ptr(part), part.stride(0),
                      torch.cuda.current_stream().cuda_stream)
        _sentinels_intact(pbuf, np.arange(M), N // 8, f"scores {kind} family {fam} M {M}")
        res.append(part.cpu())
    assert _same_bits(res[0][:17], res[1]), "the partials of a row depend on M"
