"""Host-side checks of the GEMM tests' reference and bound (no GPU): tests/gemm_ref.py agrees with
torch's float64 operators on every epilogue and under the row remap; a float32 numpy restatement of
the kernels' arithmetic stays inside gemm_bound / scores_bound with at least a factor of two to
spare; common.h's 2.6e-5 for gelu_fast holds on a dense grid; and aaclip_gemm, aaclip_gemm_scores,
aaclip_gemm_pin and aaclip_set_gemm_variant reject bad arguments without a launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aaclip import _lib, ops

import gemm_ref as GR

KINDS = ("bf16", "f16", "f32")


# ---------------------------------------------------------------------------- the reference
def _torch_ref(a, w, bias, act, resid, remap):
    v = torch.from_numpy(a).double() @ torch.from_numpy(w).double().T
    if bias is not None:
        v = v + torch.from_numpy(bias).double()
    if "qgelu" in act:
        v = v * torch.sigmoid(1.702 * v)
    elif "gelu" in act:
        v = F.gelu(v)
    if "leaky" in act:
        v = F.leaky_relu(v, 0.01)
    M = a.shape[0]
    dst = torch.arange(M)
    if remap:
        g, go, off = remap
        dst = torch.tensor([(m // g) * go + off + m % g for m in range(M)])
    if resid is not None:
        v = v + torch.from_numpy(resid).double()[dst]
    return v.numpy(), dst.numpy()


@pytest.mark.parametrize("name", list(GR.EPILOGUES))
def test_gemm_ref_agrees_with_torch_float64(name):
    has_bias, act, has_res, _, remap = GR.EPILOGUES[name]
    rm = GR.REMAP if remap else None
    a, w, bias, resid = GR.gemm_inputs(35, 64, 192, "bf16", 1, rm)
    a[:, 0] *= 4  # pre-activations out to |v| of about 6: the GELU tails
    kw = dict(bias=bias if has_bias else None, act=act, residual=resid if has_res else None, row_remap=rm)
    got, dst = GR.gemm_ref(a, w, **kw)
    ref, rdst = _torch_ref(a, w, kw["bias"], act, kw["residual"], rm)
    assert got.dtype == np.float64 and np.array_equal(dst, rdst)
    assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    if remap:  # by hand: groups of 5 land at 2..6, 9..13, ...; rows 0, 1 (mod 7) are skipped
        assert list(dst[:7]) == [2, 3, 4, 5, 6, 9, 10] and not set(dst % 7) & {0, 1}


def test_activation_combinations_and_round16_against_torch():
    v = np.linspace(-9, 9, 2001)
    for act in GR.ACTS:
        t = torch.from_numpy(v)
        if "qgelu" in act:
            t = t * torch.sigmoid(1.702 * t)
        elif "gelu" in act:
            t = F.gelu(t)
        if "leaky" in act:
            t = F.leaky_relu(t, 0.01)
        assert np.abs(GR.act64(v, act) - t.numpy()).max() <= 1e-14, act
    x = np.random.default_rng(5).standard_normal(4096) * np.logspace(-8, 4, 4096)
    x[:4] = [1.00390625, 1.01171875, 2.0 ** -25, 3 * 2.0 ** -25]  # bf16 ties (to even); fp16 subnormal ties
    for kind, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        ref = torch.from_numpy(x).to(dt).double().numpy()
        assert np.array_equal(GR.round16(x, kind), ref), kind
        assert np.all(np.abs(ref - x) <= GR.half_ulp(x, kind)), kind
    assert GR.half_ulp(1.5, "bf16") == 2.0 ** -8 and GR.half_ulp(1.5, "f16") == 2.0 ** -11
    assert GR.half_ulp(2.0 ** -20, "f16") == 2.0 ** -25


def test_lipschitz_constants_come_from_the_functions():
    """The slopes on a dense float64 grid: GELU' peaks at sqrt(2), QuickGELU's at 1.702 x = 2.3994."""
    x = np.linspace(-12, 12, 2_400_001)
    for act, L in (("gelu", GR.L_GELU), ("qgelu", GR.L_QGELU)):
        slope = np.abs(np.diff(GR.act64(x, act)) / np.diff(x)).max()
        print(f"{act}: largest slope {slope:.6f}, constant {L}")
        assert slope <= L <= slope * 1.0001


# ---------------------------------------------------------------------------- gelu_fast's documented error
def test_gelu_fast_documented_error_holds_on_a_dense_grid():
    """common.h claims |gelu_fast - erf GELU| <= 2.6e-5 on [-12, 12]. Measured with the float32
    restatement (correctly rounded exp2 and division) on 2.4 million points: 2.5565e-5, at v = 3.08."""
    v = np.linspace(-12, 12, 2_400_001).astype(np.float32)
    err = np.abs(GR.gelu_fast32(v).astype(np.float64) - GR.act64(v.astype(np.float64), "gelu"))
    i = int(err.argmax())
    print(f"max |gelu_fast - erf GELU| = {err[i]:.4e} at v = {v[i]:.4f}")
    assert err[i] <= GR.GELU_FAST_ABS
    # the device's v_exp_f32 / v_rcp_f32 are good to 1 ulp each where numpy rounds correctly: that moves
    # y = v / (1 + 2^w) by at most 3 ulp of |y| <= 12, i.e. 4.3e-6 at the far end and 9e-7 at the maximum
    assert err[i] + 3 * GR.ULP * abs(float(v[i])) <= GR.GELU_FAST_ABS + 1e-6


def test_qgelu_fast_documented_error_in_ulp():
    """common.h gives qgelu_fast2 2 ulp against the exact form. With the float32 restatement that
    holds in ulp of the result for v >= 0 (1.4 measured) and in ulp of the argument everywhere (1.2);
    for v < 0 the rounding of the exponent's argument 1.702 log2(e) v is amplified by its size, and
    in ulp of the (tiny) result the form is off by 2.8 on [-2, 0), 4.8 on [-6, -2) and 8.4 on
    [-12, -6). gemm_bound therefore takes the 2 ulp at |v|."""
    v = np.linspace(-12, 12, 2_400_001).astype(np.float32)
    ref = GR.act64(v.astype(np.float64), "qgelu")
    err = np.abs(GR.qgelu_fast32(v).astype(np.float64) - ref)
    pos = v >= 0
    of_result = err / (GR.ULP * np.maximum(np.abs(ref), 1e-300))
    of_arg = err / (GR.ULP * np.maximum(np.abs(v), 1e-30))
    print(f"qgelu_fast2: worst error {of_result[pos].max():.2f} ulp of the result for v >= 0, "
          f"{of_result[~pos].max():.2f} for v < 0; {of_arg.max():.2f} ulp of the argument")
    assert of_result[pos].max() <= GR.QGELU_FAST_ULP and of_arg.max() <= GR.QGELU_FAST_ULP
    assert of_result[~pos].max() > GR.QGELU_FAST_ULP  # why the bound cannot use the result's ulp there


# ---------------------------------------------------------------------------- the bound leaves headroom
def _shares(err, terms):
    """Where error / bound is worst: the share of the bound each term holds there."""
    total = sum(terms.values())
    i = np.unravel_index(int((err / total).argmax()), total.shape)
    return {k: float(t[i] / total[i]) if np.ndim(t) else float(t / total[i]) for k, t in terms.items()}


@pytest.mark.parametrize("K", [64, 128, 192, 320])
@pytest.mark.parametrize("kind", KINDS)
def test_float32_restatement_stays_inside_the_bound(kind, K):
    """The kernels' arithmetic in float32 numpy (gemm_ref.gemm32 / epilogue32) against the float64
    reference, on the GPU test's shape classes: every K-step count of the 16-bit kernels (K / 4 for
    the fp32 kernel, whose K-step is 16), every epilogue, fp32 and 16-bit outputs. Worst
    |error| / bound into an fp32 C: 0.041 for 16-bit operands (f16, K = 64; 0.002 at K = 320: the
    worst-case accumulation term grows with K, the error with its root) and 0.137 for fp32 operands
    (K = 16). With erf GELU the 16-bit kernels' ratio is 0.60 at K = 64, because gelu_fast's 2.6e-5
    is a form error that is reached (2.56e-5), not a rounding estimate; beside it the same 0.041. Into
    a 16-bit C the rounding of the output is nearly the whole error and the bound allows exactly half
    an ulp: up to 0.999. So everything in the bound that estimates rounding leaves the kernels
    (another order inside a slice, 1-ulp exp and rcp) more than a factor of two."""
    in16 = kind != "f32"
    Kk = K if in16 else K // 4
    worst32 = worst16 = worst_round = 0.0
    for name, (has_bias, act, has_res, has_aux, remap) in GR.EPILOGUES.items():
        rm = GR.REMAP if remap else None
        a, w, bias, resid = GR.gemm_inputs(35, 64, Kk, kind, 2, rm)
        kw = dict(bias=bias if has_bias else None, act=act, residual=resid if has_res else None, row_remap=rm)
        ref, _ = GR.gemm_ref(a, w, **kw)
        y = GR.epilogue32(GR.gemm32(a, w, in16=in16), in16=in16, **kw)
        err = np.abs(y.astype(np.float64) - ref)
        tol = GR.gemm_bound(a, w, in16=in16, out="f32", **kw)
        terms = GR.bound_terms(a, w, in16=in16, out="f32", **kw)
        assert np.allclose(sum(terms.values()), tol, rtol=1e-12, atol=0)
        r32 = (err / tol).max()
        worst32 = max(worst32, r32)
        out16 = "bf16" if kind == "f32" else kind
        y16 = GR.round16(y, out16)
        r16 = (np.abs(y16 - ref) / GR.gemm_bound(a, w, in16=in16, out=out16, **kw)).max()
        worst16 = max(worst16, r16)
        sh = _shares(err, terms)
        print(f"{kind} K {Kk} {name}: float32 restatement / bound {r32:.3f} (fp32 out), {r16:.3f} ({out16} out); "
              + ", ".join(f"{k} {v:.3f}" for k, v in sh.items() if v > 0))
        # gelu_fast's 2.6e-5 is a form error that IS reached (2.56e-5), not a rounding estimate: the
        # factor of two is asked of everything else in the bound
        form = GR.GELU_FAST_ABS if in16 and act == "gelu" else 0.0
        r_round = (np.maximum(err - form, 0) / (tol - form)).max()
        worst_round = max(worst_round, r_round)
        assert r32 <= 1.0 and r_round <= 0.5, name
        assert r16 <= 1.0, name  # the rounding term is exact, not an estimate: half an ulp is reached
    print(f"{kind} K {Kk}: worst {worst32:.3f} (fp32 out; {worst_round:.3f} beside gelu_fast's form error), "
          f"{worst16:.3f} (16-bit out)")


def test_bound_refuses_what_it_must():
    """One K-step dropped, a bias column off by four, the residual of the neighbouring row, the tanh GELU:
    each is outside the bound by a wide margin somewhere."""
    a, w, bias, resid = GR.gemm_inputs(35, 64, 192, "bf16", 3)
    ref, _ = GR.gemm_ref(a, w, bias=bias, act="gelu", residual=resid)
    tol = GR.gemm_bound(a, w, bias=bias, act="gelu", residual=resid)
    over = lambda y: (np.abs(y - ref) / tol).max()
    assert over(GR.gemm_ref(a[:, :128], w[:, :128], bias=bias, act="gelu", residual=resid)[0]) > 100
    assert over(GR.gemm_ref(a, w, bias=np.roll(bias, 4), act="gelu", residual=resid)[0]) > 100
    assert over(GR.gemm_ref(a, w, bias=bias, act="gelu", residual=np.roll(resid, 1, 0))[0]) > 100
    v = (a.astype(np.float64) @ w.astype(np.float64).T) + bias
    tanh = 0.5 * v * (1 + np.tanh(np.sqrt(2 / np.pi) * (v + 0.044715 * v ** 3))) + resid
    assert over(tanh) > 2


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_scores_restatement_stays_inside_the_bound(kind):
    """float32 partials of the float32 restatement's v against scores_ref: worst error / bound 0.08."""
    for K, N, tp, act in ((64, 256, 64, "none"), (192, 512, 128, "leaky")):
        a, w, _, _ = GR.gemm_inputs(35, N, K, kind, 4)
        T = GR.anchors(tp)
        v, _ = GR.gemm_ref(a, w, act=act)
        ref = GR.scores_ref(v, T, tp)
        tol = GR.scores_bound(v, GR.gemm_bound(a, w, act=act), T, tp)
        got = GR.scores32(GR.epilogue32(GR.gemm32(a, w), act=act), T, tp).astype(np.float64)
        assert ref.shape == (35, N // 32, 4) and np.all(ref[..., 3] == 0) and np.all(tol[..., 3] == 0)
        ratio = (np.abs(got - ref)[..., :3] / tol[..., :3]).max()
        print(f"{kind} scores K {K} N {N}: float32 restatement / bound {ratio:.3f}")
        assert ratio <= 0.5
        # by hand: group 1 of row 0
        cols = np.arange(32, 64)
        assert np.isclose(ref[0, 1, 1], (v[0, cols] * T[cols % tp, 0].astype(np.float64)).sum(), rtol=1e-13)
        if N > tp:  # the anchors wrap at t_period: the first group past it uses T[0..31] again
            g = tp // 32
            assert np.isclose(ref[0, g, 2], (v[0, tp:tp + 32] * T[:32, 1].astype(np.float64)).sum(), rtol=1e-13)


# ---------------------------------------------------------------------------- C ABI
P, Q, R_, S4, S5, S6, S7 = (ctypes.c_void_p(a << 20) for a in range(1, 8))
F32, BF16, F16, FP8 = _lib.F32, _lib.BF16, _lib.F16, _lib.FP8
BIAS, GELU, LEAKY, RESID, AUX, QGELU = (_lib.EPI_BIAS, _lib.EPI_GELU, _lib.EPI_LEAKY, _lib.EPI_RESID,
                                        _lib.EPI_AUX_BF16, _lib.EPI_QGELU)


def _off(p, n):
    return ctypes.c_void_p(p.value + n)


def _bad(fn, good):
    """Call fn with some of the well-formed arguments replaced. Every call here passes M = 0 unless it
    replaces M, so a call the entry accepts returns AACLIP_OK before any launch."""
    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    return bad


def _gemm_good(in_dtype, out_dtype, N=128, K=64, epi=BIAS | RESID | AUX):
    # (in, out, M, N, K, A, lda, W, ldw, C, ldc, epilogue, bias, residual, ldr, aux, ldaux, rg, rgo, roff, stream)
    return [in_dtype, out_dtype, 0, N, K, P, K, Q, K, R_, N, epi, S4, S5, N, S6, N, 0, 0, 0, None]


@pytest.mark.parametrize("in_dtype", [BF16, F16, F32])
def test_gemm_rejects_bad_arguments_without_a_launch(in_dtype):
    lib = _lib.lib()
    bad = _bad(lib.aaclip_gemm, _gemm_good(in_dtype, F32))
    assert bad() == 0                                              # the well-formed call, M = 0
    assert bad(a6=56) == 1 and bad(a6=68) == 1 and bad(a6=72) == 0   # lda < K; lda % 8
    assert bad(a8=56) == 1 and bad(a8=68) == 1 and bad(a8=72) == 0   # ldw
    assert bad(a10=120) == 1 and bad(a10=130) == 1 and bad(a10=132) == 0  # ldc < N; fp32 C: % 4
    for i in (5, 7, 9, 12):                                        # A, W, C, bias off 16 bytes
        assert bad(**{f"a{i}": _off(P, 8)}) == 1 and bad(**{f"a{i}": _off(P, 4)}) == 1, i
    assert all(bad(**{f"a{i}": None}) == 1 for i in (5, 7, 9))
    assert bad(a12=None) == 1                                      # bias flag without a bias
    assert bad(a13=None) == 1 and bad(a14=120) == 1 and bad(a14=130) == 1 and bad(a14=132) == 0   # residual
    assert bad(a15=None) == 1 and bad(a16=120) == 1 and bad(a16=132) == 1 and bad(a16=136) == 0   # aux: % 8
    assert bad(a11=GELU | QGELU) == 1 and bad(a11=64) == 1 and bad(a11=BIAS | 128) == 1 and bad(a11=-1) == 1
    assert bad(a17=5, a18=4) == 1 and bad(a17=-1) == 1 and bad(a17=5, a18=5) == 0
    assert bad(a2=-1) == 1 and bad(a3=0) == 1 and bad(a4=0) == 1
    assert bad(a0=FP8) == 1 and bad(a0=7) == 1 and bad(a1=FP8) == 1
    other16 = F16 if in_dtype == BF16 else BF16
    if in_dtype == F32:
        assert bad(a1=F16) == 1 and bad(a1=BF16, a10=136) == 0     # fp32 operands: C is fp32 or bf16
    else:
        assert bad(a1=other16) == 1 and bad(a1=in_dtype) == 0


@pytest.mark.parametrize("in_dtype", [BF16, F16, F32])
def test_gemm_shape_rules_hold_for_an_empty_batch(in_dtype):
    """M = 0 returns AACLIP_OK only for a shape a non-empty batch would accept."""
    lib = _lib.lib()
    bad = _bad(lib.aaclip_gemm, _gemm_good(in_dtype, F32, epi=0))
    if in_dtype == F32:
        assert bad(a3=64, a10=64) == 0 and bad(a4=16, a6=16, a8=16) == 0
        assert bad(a3=96, a10=96) == 1 and bad(a3=32, a10=32) == 1      # N % 64
        assert bad(a4=24, a6=24, a8=24) == 1 and bad(a4=8, a6=8, a8=8) == 1   # K % 16
    else:
        assert bad(a3=256, a10=256) == 0
        assert bad(a3=64, a10=64) == 1 and bad(a3=192, a10=192) == 1    # N % 128
        assert bad(a4=32, a6=32, a8=32) == 1 and bad(a4=96, a6=96, a8=96) == 1  # K % 64


@pytest.mark.parametrize("in_dtype", [BF16, F16])
def test_gemm_requires_16_byte_rows_for_a_16_bit_output(in_dtype):
    """A 16-bit C and the aux copy leave as 16-byte stores: their leading dimensions are multiples of
    8 elements (an fp32 C keeps % 4)."""
    lib = _lib.lib()
    bad = _bad(lib.aaclip_gemm, _gemm_good(in_dtype, in_dtype))
    assert bad() == 0
    assert bad(a10=132) == 1 and bad(a10=140) == 1 and bad(a10=136) == 0
    assert bad(a16=132) == 1 and bad(a16=136) == 0
    bad = _bad(lib.aaclip_gemm, _gemm_good(F32, BF16, epi=0))
    assert bad(a10=132) == 1 and bad(a10=136) == 0
    # the Python wrapper says the same before it calls
    aux = torch.zeros(4, 132, dtype=torch.bfloat16)[:, :128]
    with pytest.raises(ValueError, match="multiple of 8"):
        ops._epilogue_flags(128, 4, None, False, False, None, aux)
    ok = torch.zeros(4, 136, dtype=torch.bfloat16)[:, :128]
    assert ops._epilogue_flags(128, 4, None, False, False, None, ok) == (AUX, 0, 136)


def test_gemm_scores_rejects_bad_arguments_without_a_launch():
    lib = _lib.lib()
    # (in_dtype, M, N, K, A, lda, W, ldw, epilogue, T, t_period, part, ld_part, stream)
    bad = _bad(lib.aaclip_gemm_scores, [BF16, 0, 256, 64, P, 64, Q, 64, 0, R_, 64, S4, 32, None])
    assert bad() == 0 and bad(a0=F16) == 0 and bad(a8=LEAKY) == 0
    assert bad(a0=F32) == 1 and bad(a0=FP8) == 1
    assert all(bad(**{f"a{i}": None}) == 1 for i in (4, 6, 9, 11))
    assert bad(a1=-1) == 1 and bad(a2=0) == 1 and bad(a3=0) == 1
    assert bad(a3=32, a5=32, a7=32) == 1 and bad(a3=96, a5=96, a7=96) == 1          # K % 64
    assert bad(a2=128, a12=16) == 1 and bad(a2=384, a12=48) == 1                    # N % 256
    assert bad(a10=0) == 1 and bad(a10=-64) == 1 and bad(a10=32) == 1 and bad(a10=96) == 1 and bad(a10=128) == 0
    assert bad(a12=28) == 1 and bad(a12=34) == 1 and bad(a12=36) == 0               # ld_part < N / 8; % 4
    assert bad(a5=56) == 1 and bad(a5=68) == 1 and bad(a5=72) == 0
    assert bad(a7=56) == 1 and bad(a7=68) == 1 and bad(a7=72) == 0
    for i in (4, 6, 9, 11):
        assert bad(**{f"a{i}": _off(P, 8)}) == 1, i
    assert bad(a8=BIAS) == 1 and bad(a8=GELU) == 1 and bad(a8=LEAKY | RESID) == 1 and bad(a8=64) == 1


def test_gemm_pin_and_variant_reject_what_the_dispatch_cannot_honour():
    lib = _lib.lib()
    try:
        for fam in (1, 3, 8, 9):                                   # the 256-column families
            assert lib.aaclip_gemm_pin(BF16, 5, 128, 64, fam) == 1
            assert lib.aaclip_gemm_pin(F16, 5, 384, 64, fam) == 1
            assert lib.aaclip_gemm_pin(BF16, 5, 256, 64, fam) == 0
        for fam in (2, 11):
            assert lib.aaclip_gemm_pin(BF16, 5, 128, 64, fam) == 0
        for fam in (4, 5, 6, 7, 10, 12, -1):
            assert lib.aaclip_gemm_pin(BF16, 5, 256, 64, fam) == 1
        assert lib.aaclip_gemm_pin(F32, 5, 256, 64, 2) == 1 and lib.aaclip_gemm_pin(BF16, 0, 256, 64, 2) == 1
        assert lib.aaclip_gemm_plan(BF16, 5, 256, 64) == b"gemm_bf16_kernel<128,128,2,2>"   # family 9, pinned last
    finally:
        for n in (128, 256):
            assert lib.aaclip_gemm_pin(BF16, 5, n, 64, 0) == 0
    try:
        for v in (5, 7, 10, 12, 15, -1, 4096, 16 + 5):             # the removed families, out of range
            assert lib.aaclip_set_gemm_variant(v) == 1, v
        for v in (1, 2, 3, 4, 8, 9, 11, 0):
            assert lib.aaclip_set_gemm_variant(v) == 0, v
    finally:
        lib.aaclip_set_gemm_variant(0)
