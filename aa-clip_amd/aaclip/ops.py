"""Tensor-level wrappers over the C ABI (include/aaclip.h).

torch is plumbing here: device memory, the current HIP stream, dtype tags.
Every function validates shapes/dtypes on the host (a kernel is never launched
on operands whose shapes disagree with what its grid assumes) and launches one
HIP kernel on torch's current stream. There is no eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import BF16, F16, F32, call

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def dtag(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}; expected float32, bfloat16 or float16") from None


def torch_dtype(tag: int) -> torch.dtype:
    return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[tag]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(*ts):
    """Every operand must be a device tensor on the CURRENT device: kernels launch on
    the current device's stream (and the C side keys its per-device caches on
    hipGetDevice), so a tensor on another GPU would be a wrong-device pointer. The
    engines enter `torch.cuda.device(their device)` around every launch sequence."""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("aaclip ops need device (HIP) tensors; there is no CPU path")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError(f"aaclip op operand on {t.device} but the current device is cuda:{cur}; "
                               "wrap the call in torch.cuda.device(...)")


# In-step launch probe (measurement only; None in production): an object with
# begin(kind, name, flops, nbytes) -> token and end(token), called around every
# launch of the ops below so a caller (bench.py) can put HIP timing events around
# each kernel inside a captured step. It never changes what is launched.
_probe = None


def set_probe(probe) -> None:
    global _probe
    _probe = probe


def _launch(kind: str, name, flops: float, nbytes: float, fn, *args) -> None:
    """call(fn, *args), bracketed by the probe when one is set."""
    if _probe is None:
        call(fn, *args)
        return
    tok = _probe.begin(kind, name() if callable(name) else name, flops, nbytes)
    call(fn, *args)
    _probe.end(tok)


def _rowmajor(t: torch.Tensor, name: str):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be a 2-D tensor with unit column stride")


# ------------------------------------------------------------------------ GEMM
def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias=None, gelu=False, leaky=False,
         residual=None, aux=None, row_group=0, row_group_out=0, row_offset=0) -> torch.Tensor:
    """out = epilogue(a @ w.T) — a [M,K], w [N,K] (same dtype), out [M', N].
    gelu: True = exact erf GELU (nn.GELU), "quick" = QuickGELU x*sigmoid(1.702x)
    (reference model/transformer.py:46-49)."""
    _dev(a, w, out, bias, residual, aux)
    for t, n in ((a, "a"), (w, "w"), (out, "out")):
        _rowmajor(t, n)
    if a.dtype != w.dtype:
        raise TypeError("gemm operands must share a dtype")
    if out.dtype not in (torch.float32, a.dtype) and not (a.dtype == torch.float32 and out.dtype == torch.bfloat16):
        raise TypeError("gemm output must be float32 or the operands' 16-bit dtype")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or out.shape[1] != N:
        raise ValueError(f"gemm shape mismatch a{tuple(a.shape)} w{tuple(w.shape)} out{tuple(out.shape)}")
    rows_out = M if row_group == 0 else ((M - 1) // row_group) * row_group_out + row_offset + (M - 1) % row_group + 1
    if out.shape[0] < rows_out or (row_group and M % row_group):
        raise ValueError("gemm output rows too small for the row remap")
    if out.element_size() == 2 and out.stride(0) % 8:
        raise ValueError("gemm: a 16-bit output's row stride must be a multiple of 8 elements (16-byte stores)")
    epi, ldr, ldaux = _epilogue_flags(N, rows_out, bias, gelu, leaky, residual, aux,
                                      aux_dtype=torch.float16 if a.dtype == torch.float16 else torch.bfloat16)
    kind = f"gemm N{N} K{K}" + (" leaky" if leaky else "") + (" qgelu" if gelu == "quick" else " gelu" if gelu else "") + (" resid" if residual is not None else "")
    nbytes = (M * K + N * K) * a.element_size() + rows_out * N * out.element_size() * (2 if residual is not None else 1)
    _launch(kind, lambda: gemm_plan(dtag(a), M, N, K) if a.dtype != torch.float32 else "gemm_f32_kernel",
            2.0 * M * N * K, nbytes, "aaclip_gemm", dtag(a), dtag(out), M, N, K, _ptr(a), a.stride(0), _ptr(w),
            w.stride(0), _ptr(out), out.stride(0), epi, _ptr(bias), _ptr(residual), ldr, _ptr(aux), ldaux,
            row_group, row_group_out, row_offset, _stream())
    return out


# tile families aaclip_gemm_pin accepts (include/aaclip.h): 8-phase 256x256, 320x256,
# 256x256, 128x128, 256x128, 64x64 (the two-workgroup family 10 was removed in round 5)
GEMM_FAMILIES = (3, 8, 1, 9, 2, 11)
_tuned = {}


def _family_applies(fam: int, N: int, K: int) -> bool:
    """The shapes aaclip_gemm_pin / choose16 honour a family on (else it falls back)."""
    if fam in (1, 3, 8, 9):
        return N % 256 == 0
    if fam == 11:
        return N % 64 == 0
    return True  # 0 (the unpinned per-shape heuristic) and 2


def pin_gemm(dtype: int, M: int, N: int, K: int, family: int) -> None:
    """aaclip_gemm_pin: launch tile family `family` (GEMM_FAMILIES; 0 = back to the
    per-shape heuristic) for every 16-bit GEMM of this (dtype tag, M, N, K)."""
    call("aaclip_gemm_pin", dtype, M, N, K, family)


class concurrent_gemms:
    """Context manager: aaclip_gemm_concurrent for the calling thread while image chunks
    are enqueued on concurrent streams (block-GEMM shapes that fill a round of the CUs
    take the 8-phase kernel; bit-identical). Restores the previous state on exit."""

    def __init__(self, on: bool = True):
        self.on = int(bool(on))
        self.prev = ctypes.c_int(0)

    def __enter__(self):
        call("aaclip_gemm_concurrent", self.on, ctypes.byref(self.prev))
        return self

    def __exit__(self, *exc):
        call("aaclip_gemm_concurrent", self.prev.value, None)
        return False


def gemm_plan(tag: int, M: int, N: int, K: int) -> str:
    """Kernel name aaclip_gemm launches for this shape on this thread (reports)."""
    return _lib.lib().aaclip_gemm_plan(tag, M, N, K).decode()


def tune_gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, reps: int = 3, **epilogue) -> int:
    """Measure every tile family on these operands with this epilogue (HIP events on the
    current stream) and pin the fastest for the shape (aaclip_gemm_pin). The families
    accumulate K in the same order, so the pin changes speed, never bits. Host-side
    setup only (it synchronises): never call it while a hipGraph is being captured.
    Returns the pinned family; shapes already tuned in this process are skipped."""
    if a.dtype not in (torch.bfloat16, torch.float16):
        return 0
    M, K = a.shape
    N = w.shape[0]
    key = (dtag(a), M, N, K)
    if key in _tuned:
        return _tuned[key]
    st = torch.cuda.current_stream()
    best, best_t = 0, float("inf")
    try:
        # family 0 = unpinned: the heuristic's own choice (e.g. the 64x64 tiles it takes for
        # single-image shapes) is a candidate, so a pin is never slower than no pin
        for fam in (0,) + GEMM_FAMILIES:
            if not _family_applies(fam, N, K):
                continue
            call("aaclip_gemm_pin", key[0], M, N, K, fam)
            gemm(a, w, out, **epilogue)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps):
                gemm(a, w, out, **epilogue)
            e1.record(st)
            e1.synchronize()
            t = e0.elapsed_time(e1)
            if t < best_t:
                best, best_t = fam, t
    finally:
        call("aaclip_gemm_pin", key[0], M, N, K, best)
    _tuned[key] = best
    return best


FP8 = torch.float8_e4m3fn  # OCP e4m3 (gfx950), one byte per element


def quant_fp8_rows(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor) -> None:
    """Per-row e4m3 quantisation: scale[r] = max|x[r]|/448, q = RNE(x/scale)."""
    _dev(x, q, scale)
    _rowmajor(x, "x")
    _rowmajor(q, "q")
    if q.dtype != FP8 or scale.dtype != torch.float32 or not scale.is_contiguous():
        raise TypeError("q must be float8_e4m3fn and scale contiguous fp32")
    rows, cols = x.shape
    if tuple(q.shape) != (rows, cols) or scale.numel() < rows:
        raise ValueError("quant_fp8_rows shape mismatch")
    call("aaclip_quant_fp8_rows", dtag(x), _ptr(x), x.stride(0), _ptr(q), q.stride(0), _ptr(scale), rows, cols,
         _stream())


def gemm_fp8(a: torch.Tensor, a_scale: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, out: torch.Tensor, *,
             bias=None, gelu=False, leaky=False, residual=None, aux=None, row_group=0, row_group_out=0,
             row_offset=0) -> torch.Tensor:
    """out = epilogue(a_scale[:,None] * w_scale[None,:] * (a @ w.T)) with e4m3 a [M,K], w [N,K]."""
    _dev(a, a_scale, w, w_scale, out, bias, residual, aux)
    for t, n in ((a, "a"), (w, "w"), (out, "out")):
        _rowmajor(t, n)
    if a.dtype != FP8 or w.dtype != FP8:
        raise TypeError("gemm_fp8 operands must be float8_e4m3fn")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or out.shape[1] != N or a_scale.numel() < M or w_scale.numel() != N:
        raise ValueError(f"gemm_fp8 shape mismatch a{tuple(a.shape)} w{tuple(w.shape)} out{tuple(out.shape)}")
    if a_scale.dtype != torch.float32 or w_scale.dtype != torch.float32:
        raise TypeError("fp8 scales must be fp32")
    rows_out = M if row_group == 0 else ((M - 1) // row_group) * row_group_out + row_offset + (M - 1) % row_group + 1
    if out.shape[0] < rows_out or (row_group and M % row_group):
        raise ValueError("gemm output rows too small for the row remap")
    epi, ldr, ldaux = _epilogue_flags(N, rows_out, bias, gelu, leaky, residual, aux)
    call("aaclip_gemm_fp8", dtag(out), M, N, K, _ptr(a), a.stride(0), _ptr(a_scale), _ptr(w), w.stride(0),
         _ptr(w_scale), _ptr(out), out.stride(0), epi, _ptr(bias), _ptr(residual), ldr, _ptr(aux), ldaux,
         row_group, row_group_out, row_offset, _stream())
    return out


def mx_scales(rows: int, cols: int, device, ld: int = None) -> torch.Tensor:
    """e8m0 scale buffer of an MX fp8 tensor [rows, cols]: [cols/128, ld, 2] uint8
    (one byte per (row, 64-column block); the two blocks of a 128-K step adjacent).
    ld defaults to rows rounded up to even (the MX GEMM moves scales as dwords)."""
    return torch.empty(cols // 128, ld or (rows + 1) // 2 * 2, 2, device=device, dtype=torch.uint8)


def quant_fp8_mx(x: torch.Tensor, q: torch.Tensor, sc: torch.Tensor) -> None:
    """MX fp8: q = e4m3(x * 2^-e), e8m0 e per (row, 64-column block) into sc [cols/128, ld, 2]."""
    _dev(x, q, sc)
    _rowmajor(x, "x")
    _rowmajor(q, "q")
    rows, cols = x.shape
    if q.dtype != FP8 or sc.dtype != torch.uint8 or tuple(q.shape) != (rows, cols):
        raise TypeError("q must be float8_e4m3fn [rows, cols], sc uint8")
    if sc.dim() != 3 or sc.shape[0] != cols // 128 or sc.shape[1] < rows or sc.shape[2] != 2 or not sc.is_contiguous():
        raise ValueError("sc must be contiguous uint8 [cols/128, ld >= rows, 2]")
    call("aaclip_quant_fp8_mx", dtag(x), _ptr(x), x.stride(0), _ptr(q), q.stride(0), _ptr(sc), sc.shape[1],
         rows, cols, _stream())


def gemm_fp8mx(a: torch.Tensor, a_sc: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, out: torch.Tensor, *,
               out_sc=None, bias=None, gelu=False, leaky=False, residual=None, aux=None) -> torch.Tensor:
    """out = epilogue(w_scale[None,:] * (MX-dequant(a) @ w.T)); a: e4m3 [M,K] with e8m0 block scales
    a_sc [K/128, ld, 2]; out fp32 / bf16, or e4m3 (then out_sc receives its MX scales)."""
    _dev(a, a_sc, w, w_scale, out, out_sc, bias, residual, aux)
    for t, n in ((a, "a"), (w, "w"), (out, "out")):
        _rowmajor(t, n)
    if a.dtype != FP8 or w.dtype != FP8:
        raise TypeError("gemm_fp8mx operands must be float8_e4m3fn")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or out.shape[1] != N or out.shape[0] < M or w_scale.numel() != N:
        raise ValueError(f"gemm_fp8mx shape mismatch a{tuple(a.shape)} w{tuple(w.shape)} out{tuple(out.shape)}")
    if a_sc.dtype != torch.uint8 or a_sc.dim() != 3 or a_sc.shape[0] != K // 128 or a_sc.shape[1] < M or \
            a_sc.shape[1] % 2:
        raise ValueError("a_sc must be uint8 [K/128, ld >= M (even), 2]")
    if out.dtype == FP8:
        if out_sc is None or out_sc.shape[0] != N // 128 or out_sc.shape[1] < M:
            raise ValueError("fp8 output needs out_sc uint8 [N/128, ld >= M, 2]")
        odt = _lib.FP8
    else:
        odt = dtag(out)
    epi, ldr, ldaux = _epilogue_flags(N, M, bias, gelu, leaky, residual, aux)
    kind = f"gemm8 N{N} K{K}" + (" gelu" if gelu else "") + (" resid" if residual is not None else "")
    nbytes = M * K + N * K + M * N * out.element_size() * (2 if residual is not None else 1)
    _launch(kind, "gemm_fp8mx_8ph_kernel", 2.0 * M * N * K, nbytes, "aaclip_gemm_fp8mx", odt, M, N, K, _ptr(a),
            a.stride(0), _ptr(a_sc), a_sc.shape[1], _ptr(w), w.stride(0), _ptr(w_scale), _ptr(out), out.stride(0),
            epi, _ptr(bias), _ptr(residual), ldr, _ptr(aux), ldaux, _ptr(out_sc),
            0 if out_sc is None else out_sc.shape[1], _stream())
    return out


def _epilogue_flags(N, rows_out, bias, gelu, leaky, residual, aux, aux_dtype=torch.bfloat16):
    epi = 0
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != N:
            raise ValueError("bias must be fp32 [N]")
        epi |= _lib.EPI_BIAS
    if gelu not in (False, True, "quick"):
        raise ValueError("gelu must be False, True (erf GELU, nn.GELU) or 'quick' (QuickGELU)")
    if gelu:
        epi |= _lib.EPI_QGELU if gelu == "quick" else _lib.EPI_GELU
    if leaky:
        epi |= _lib.EPI_LEAKY
    ldr = 0
    if residual is not None:
        _rowmajor(residual, "residual")
        if residual.dtype != torch.float32 or residual.shape[1] != N or residual.shape[0] < rows_out:
            raise ValueError("residual must be fp32 [rows, N]")
        epi |= _lib.EPI_RESID
        ldr = residual.stride(0)
    ldaux = 0
    if aux is not None:
        _rowmajor(aux, "aux")
        if aux.dtype != aux_dtype or aux.shape[1] != N or aux.shape[0] < rows_out:
            raise ValueError(f"aux must be {aux_dtype} [rows, N] (fp16 for fp16 operands, else bf16)")
        if aux.stride(0) % 8:
            raise ValueError("aux: the row stride must be a multiple of 8 elements (16-byte stores)")
        epi |= _lib.EPI_AUX_BF16
        ldaux = aux.stride(0)
    return epi, ldr, ldaux


# ------------------------------------------------------------------------ attention
def attention(qkv: torch.Tensor, out: torch.Tensor, batch: int, seq: int, heads: int,
              causal: bool = False, out_sc=None, q_prescaled: bool = False) -> torch.Tensor:
    """out = MHA core of packed qkv; out fp8 (e4m3) + out_sc = MX output (bf16 qkv only).
    q_prescaled: the q columns already carry log2(e)/sqrt(64) (bf16 / fp16 qkv only)."""
    _dev(qkv, out, out_sc)
    flags = (_lib.ATTN_CAUSAL if causal else 0) | (_lib.ATTN_Q_PRESCALED if q_prescaled else 0)
    if q_prescaled and qkv.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("q_prescaled needs bf16 or fp16 qkv")
    hd = 64
    if qkv.shape != (batch * seq, 3 * heads * hd) or out.shape != (batch * seq, heads * hd):
        raise ValueError("attention shape mismatch")
    if not (qkv.is_contiguous() and out.is_contiguous()):
        raise ValueError("attention tensors must be contiguous")
    if out.dtype == FP8:
        if qkv.dtype != torch.bfloat16 or out_sc is None or out_sc.dtype != torch.uint8 or \
                out_sc.shape[0] != heads // 2 or out_sc.shape[1] < batch * seq:
            raise ValueError("fp8 attention output needs bf16 qkv and MX scales [heads/2, ld, 2]")
        call("aaclip_attention", _lib.FP8, _ptr(qkv), _ptr(out), batch, seq, heads, hd, flags,
             _ptr(out_sc), out_sc.shape[1], _stream())
        return out
    if qkv.dtype != out.dtype:
        raise ValueError("attention tensors must share a dtype")
    flops = 4.0 * batch * heads * seq * seq * hd / (2 if causal else 1)
    _launch("attention", {torch.float32: "attn_f32_kernel"}.get(qkv.dtype, "attn_bf16_kernel"), flops,
            qkv.numel() * qkv.element_size() + out.numel() * out.element_size(), "aaclip_attention", dtag(qkv),
            _ptr(qkv), _ptr(out), batch, seq, heads, hd, flags, None, 0, _stream())
    return out


VV_MAX_BATCH = _lib.VV_MAX_BATCH


def vv_attention(v: torch.Tensor, out: torch.Tensor, batch: int, n_tok: int, heads: int) -> torch.Tensor:
    """out = v-v "surgery" attention ACROSS THE IMAGES of the batch, per token position and
    head (aaclip_vv_attention; reference model/transformer.py:125-152 on the tower's
    [L, N, D] layout). v: [batch*n_tok, heads*64] rows with unit column stride: its own
    buffer or a column view (the V third) of a packed qkv buffer; out likewise, same
    dtype, not overlapping v."""
    _dev(v, out)
    _rowmajor(v, "v")
    _rowmajor(out, "out")
    hd = 64
    if v.shape != (batch * n_tok, heads * hd) or out.shape != v.shape:
        raise ValueError("vv_attention shape mismatch")
    if v.dtype != out.dtype:
        raise ValueError("vv_attention tensors must share a dtype")
    if not 1 <= batch <= VV_MAX_BATCH:
        raise ValueError(f"vv_attention couples the images of a batch: 1..{VV_MAX_BATCH} images, got {batch}")
    vec = 16 // v.element_size()
    for t, n in ((v, "v"), (out, "out")):
        if t.stride(0) < heads * hd or t.stride(0) % vec or t.data_ptr() % 16:
            raise ValueError(f"vv_attention: {n} needs a row stride >= {heads * hd} that is a multiple of {vec} "
                             "elements, and a 16-byte aligned start")
    lo, hi = v.data_ptr(), v.data_ptr() + ((v.shape[0] - 1) * v.stride(0) + v.shape[1]) * v.element_size()
    olo, ohi = out.data_ptr(), out.data_ptr() + ((out.shape[0] - 1) * out.stride(0) + out.shape[1]) * out.element_size()
    if lo < ohi and olo < hi:
        raise ValueError("vv_attention: out must not overlap v")
    nbytes = 2 * v.shape[0] * v.shape[1] * v.element_size()
    _launch("vv_attention", "vv_attention_kernel", 4.0 * batch * batch * hd * n_tok * heads, nbytes,
            "aaclip_vv_attention", dtag(v), _ptr(v), v.stride(0), _ptr(out), out.stride(0), batch, n_tok, heads, hd,
            _stream())
    return out


# ------------------------------------------------------------------------ rows
def im2col(img: torch.Tensor, cols: torch.Tensor, patch: int) -> torch.Tensor:
    _dev(img, cols)
    B, C, S, S2 = img.shape
    g = S // patch
    if S != S2 or img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError("image must be contiguous fp32 [B,C,S,S]")
    if cols.shape[0] != B * g * g or not cols.is_contiguous():
        raise ValueError("cols shape mismatch")
    _launch("im2col", "im2col_band_kernel", 0.0, img.numel() * 4 + cols.numel() * cols.element_size(), "aaclip_im2col",
            dtag(cols), _ptr(img), _ptr(cols), B, C, S, patch, cols.shape[1], _stream())
    return cols


def _mx_out(t, sc, rows):
    """(dtype tag, scale ptr, ld) for an LN output: fp8 MX (t e4m3 + sc e8m0) or plain."""
    if t is not None and t.dtype == FP8:
        if sc is None or sc.dtype != torch.uint8 or sc.dim() != 3 or sc.shape[1] < rows or not t.is_contiguous():
            raise ValueError("fp8 LayerNorm output needs a contiguous e4m3 tensor and MX scales [w/128, ld, 2]")
        return _lib.FP8, _ptr(sc), sc.shape[1]
    return (dtag(t) if t is not None else None), None, 0


def _rows32(t, name, shape=None):
    """A contiguous fp32 [rows, width] operand: the fused row kernels stride by the width alone."""
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous() \
            or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name} must be contiguous fp32 [rows, width]" + (f" {list(shape)}" if shape is not None else ""))


def _rows_out(t, name, shape):
    """A contiguous [rows, width] output (its dtype is checked by dtag / _mx_out)."""
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous {list(shape)}")


def _ln_pair(ln, name, width):
    if len(ln) != 2:
        raise ValueError(f"{name} must be a (weight, bias) pair")
    _f32c(ln[0], name + " weight", (width,))
    _f32c(ln[1], name + " bias", (width,))


def _tokens32(tokens):
    if tokens.dim() != 2 or tokens.dtype != torch.int32 or not tokens.is_contiguous():
        raise ValueError("tokens must be contiguous int32 [n_seq, ctx]")


def embed_ln(x, cls, pos, ln_pre, ln1, h, batch, n_tok, h_sc=None):
    _dev(x, h, cls, pos, *ln_pre, *ln1)
    _rows32(x, "x")
    width = x.shape[1]
    if x.shape[0] != batch * n_tok or h.shape != x.shape or pos.shape != (n_tok, width):
        raise ValueError("embed_ln shape mismatch")
    _rows_out(h, "h", x.shape)
    _f32c(cls, "cls", (width,))
    _rows32(pos, "pos")
    _ln_pair(ln_pre, "ln_pre", width)
    _ln_pair(ln1, "ln1", width)
    od, scp, ld = _mx_out(h, h_sc, x.shape[0])
    _launch("embed_ln", "embed_ln_kernel", 0.0, x.numel() * 4 * 2 + h.numel() * h.element_size(), "aaclip_embed_ln",
            od, _ptr(x), _ptr(cls), _ptr(pos), _ptr(ln_pre[0]), _ptr(ln_pre[1]), _ptr(ln1[0]), _ptr(ln1[1]),
            _ptr(h), batch, n_tok, width, scp, ld, _stream())


def block_tail(x, n_tok, *, u=None, adapt_weight=0.0, ln=None, h=None, post=None, tap=None, out_dtype=None,
               h_sc=None):
    _dev(x, u, h, tap, *(ln or ()), *(post or ()))
    _rows32(x, "x")
    rows, width = x.shape
    if u is not None:
        _rows32(u, "adapter output u", x.shape)
    if h is not None:
        _rows_out(h, "h", x.shape)
        if not ln:
            raise ValueError("h needs the (weight, bias) pair ln")
    if tap is not None:
        if n_tok < 2 or rows % n_tok or not post:
            raise ValueError("a tap needs post, n_tok > 1 and rows a multiple of n_tok")
        _rows_out(tap, "tap", (rows // n_tok * (n_tok - 1), width))
    if ln:
        _ln_pair(ln, "ln", width)
    if post:
        _ln_pair(post, "post", width)
    od, scp, ld = _mx_out(h, h_sc, rows)
    if od is None:
        od = dtag(tap) if tap is not None else F32
    if h is not None and tap is not None and h.dtype != tap.dtype and not (h.dtype == FP8 and tap.dtype == torch.bfloat16):
        raise ValueError("h and tap must share a dtype (or h fp8 MX with bf16 taps)")
    nb = rows * width * 4 * (3 if u is not None else 2) + (rows * width * h.element_size() if h is not None else 0) \
        + (tap.numel() * tap.element_size() if tap is not None else 0)
    _launch("block_tail", "block_tail_kernel", 0.0, nb, "aaclip_block_tail", od, _ptr(x), _ptr(u), float(adapt_weight),
         _ptr(ln[0]) if ln else None, _ptr(ln[1]) if ln else None, _ptr(h),
         _ptr(post[0]) if post else None, _ptr(post[1]) if post else None, _ptr(tap),
         rows, n_tok, width, scp, ld, _stream())


def layernorm(x, w, b, y, y_sc=None):
    _dev(x, y, w, b)
    _rowmajor(x, "x")
    _rowmajor(y, "y")
    if x.shape != y.shape or x.dtype != torch.float32:
        raise ValueError("layernorm shape/dtype mismatch")
    _f32c(w, "layernorm weight", (x.shape[1],))
    _f32c(b, "layernorm bias", (x.shape[1],))
    od, scp, ld = _mx_out(y, y_sc, x.shape[0])
    _launch("layernorm", "layernorm_kernel", 0.0, x.numel() * 4 + y.numel() * y.element_size(), "aaclip_layernorm",
            od, _ptr(x), x.stride(0), _ptr(w), _ptr(b), _ptr(y), y.stride(0), x.shape[0], x.shape[1], scp, ld,
            _stream())
    return y


def text_embed_ln(tokens, tok_emb, pos, ln1, x, h):
    _dev(tokens, x, h, tok_emb, pos, *ln1)
    _tokens32(tokens)
    n, ctx = tokens.shape
    _rows32(tok_emb, "tok_emb")
    width = tok_emb.shape[1]
    _rows32(x, "x", (n * ctx, width))
    _rows_out(h, "h", x.shape)
    _rows32(pos, "pos")
    if pos.shape[0] < ctx or pos.shape[1] != width:
        raise ValueError("pos must be fp32 [>= ctx, width]")
    _ln_pair(ln1, "ln1", width)
    call("aaclip_text_embed_ln", dtag(h), _ptr(tokens), _ptr(tok_emb), _ptr(pos), _ptr(ln1[0]), _ptr(ln1[1]),
         _ptr(x), _ptr(h), n, ctx, x.shape[1], _stream())


def eot_ln(x, tokens, ln, y):
    _dev(x, tokens, y, *ln)
    _tokens32(tokens)
    n, ctx = tokens.shape
    _rows32(x, "x")
    if x.shape[0] != n * ctx:
        raise ValueError("eot_ln shape mismatch")
    _rows_out(y, "y", (n, x.shape[1]))
    _ln_pair(ln, "ln", x.shape[1])
    call("aaclip_eot_ln", dtag(y), _ptr(x), _ptr(tokens), _ptr(ln[0]), _ptr(ln[1]), _ptr(y), n, ctx,
         x.shape[1], _stream())
    return y


def anchor_reduce(emb: torch.Tensor, T: torch.Tensor, col: int):
    _dev(emb, T)
    _rows32(emb, "emb")
    n, dim = emb.shape
    if T.dim() != 2 or T.shape[0] != dim or T.dtype != torch.float32 or not T.is_contiguous():
        raise ValueError("T must be contiguous fp32 [dim, ncols]")
    if not 0 <= col < T.shape[1]:
        raise ValueError(f"col {col} outside T's {T.shape[1]} columns")
    if not (1 <= n <= 256 and dim <= 1024):
        raise ValueError("anchor_reduce takes 1..256 rows of at most 1024 columns")
    call("aaclip_anchor_reduce", _ptr(emb), n, dim, _ptr(T), col, T.shape[1], _stream())


def l2_normalize(x, y):
    _dev(x, y)
    _rowmajor(x, "x")
    _rowmajor(y, "y")
    if x.shape != y.shape:
        raise ValueError("l2_normalize shape mismatch")
    if x.stride(0) % 4 or y.stride(0) % 4:
        raise ValueError("l2_normalize row strides must be multiples of 4 elements")
    call("aaclip_l2_normalize", dtag(x), dtag(y), _ptr(x), x.stride(0), _ptr(y), y.stride(0),
         x.shape[0], x.shape[1], _stream())
    return y


# ------------------------------------------------------------------------ anomaly map
def _level_array(levels):
    arr = (ctypes.c_void_p * len(levels))(*[t.data_ptr() for t in levels])
    return arr


def patch_scores(levels, T, out, *, normalize=True, mode=0, group=0):
    """mode 0: out[row] = sum_l (A1 + 1 - A0)/2; mode 1 (one level): out [B, 2, group] logits."""
    _dev(*levels, T, out)
    rows, C = levels[0].shape
    for t in levels:
        _rowmajor(t, "level")
        if t.shape != (rows, C) or t.dtype != levels[0].dtype or t.stride(0) != levels[0].stride(0):
            raise ValueError("levels must share shape, dtype and stride")
    if T.shape != (C, 2) or T.dtype != torch.float32 or not T.is_contiguous():
        raise ValueError("T must be contiguous fp32 [C, 2]")
    need = rows if mode == 0 else 2 * rows
    if out.numel() < need or out.dtype != torch.float32:
        raise ValueError("patch_scores output too small")
    if mode == 1 and (group <= 0 or rows % group):
        raise ValueError("mode 1 needs group = patches per image dividing the rows")
    arr = _level_array(levels)
    call("aaclip_patch_scores", dtag(levels[0]), arr, len(levels), levels[0].stride(0), _ptr(T), rows, C,
         int(normalize), mode, group, _ptr(out), _stream())
    return out


def patch_logits(f, T, out, *, group):
    """Train-branch logits for any anchor count: out [B, n_anchor, group] = 100 * f . T."""
    _dev(f, T, out)
    _rowmajor(f, "f")
    rows, C = f.shape
    n = T.shape[1] if T.dim() == 2 else 0
    if T.dim() != 2 or T.shape[0] != C or T.dtype != torch.float32 or not T.is_contiguous():
        raise ValueError("T must be contiguous fp32 [C, n_anchor]")
    if out.numel() < rows * n or out.dtype != torch.float32 or not out.is_contiguous() or group <= 0 or rows % group:
        raise ValueError("patch_logits output / group mismatch")
    call("aaclip_patch_logits", dtag(f), _ptr(f), f.stride(0), _ptr(T), n, rows, C, group, _ptr(out), _stream())
    return out


def blur_upsample(grid, out, *, ksize, sigma, softmax=False):
    _dev(grid, out)
    B, C, g, g2 = grid.shape
    S = out.shape[-1]
    if g != g2 or out.shape != (B, C, S, S) or not grid.is_contiguous() or not out.is_contiguous():
        raise ValueError("blur_upsample shape mismatch")
    call("aaclip_blur_upsample", _ptr(grid), _ptr(out), B, C, g, S, ksize, float(sigma), int(softmax), _stream())
    return out


# ------------------------------------------------------------------------ stage-1 loss head
SEGLOSS_CHUNK = 4096   # AACLIP_SEGLOSS_CHUNK
LOGITS_BWD_ROWS = 16   # AACLIP_LOGITS_BWD_ROWS


def _f32c(t, name, shape=None):
    if t.dtype != torch.float32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name} must be contiguous fp32" + (f" {list(shape)}" if shape is not None else ""))


def _anchors(T, C, batch, n_anchor=None):
    """(t_stride, n_anchor) of shared [C, n] or per-image [batch, C, n] contiguous fp32 anchors."""
    if T.dim() not in (2, 3) or T.dtype != torch.float32 or not T.is_contiguous() or T.shape[-2] != C:
        raise ValueError("T must be contiguous fp32 [C, n_anchor] or [batch, C, n_anchor]")
    if T.dim() == 3 and T.shape[0] != batch:
        raise ValueError(f"per-image anchors need one set per image: got {T.shape[0]} for a batch of {batch}")
    n = T.shape[-1]
    if n_anchor is not None and n != n_anchor:
        raise ValueError(f"this op takes {n_anchor} anchors, got {n}")
    return (C * n if T.dim() == 3 else 0), n


def patch_logits_per_image(f, T, out, *, group):
    """Train-branch logits with shared [C, n] or per-image [B, C, n] anchors (n <= 8):
    out [B, n, group] = 100 * f[b] . T[b]. A shared T gives patch_logits' bits."""
    _dev(f, T, out)
    _rowmajor(f, "f")
    rows, C = f.shape
    if group <= 0 or rows % group:
        raise ValueError("group = patches per image must divide the rows")
    t_stride, n = _anchors(T, C, rows // group)
    if not 1 <= n <= 8:
        raise ValueError(f"patch_logits_per_image supports 1..8 anchors, got {n}")
    if out.numel() < rows * n or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("patch_logits_per_image output too small / not contiguous fp32")
    nb = rows * C * f.element_size() + T.numel() * 4 + rows * n * 4
    _launch("segloss", "patch_logits_per_image", 2.0 * rows * C * n, nb, "aaclip_patch_logits_per_image", dtag(f),
            _ptr(f), f.stride(0), _ptr(T), t_stride, n, rows, C, group, _ptr(out), _stream())
    return out


def seg_loss_workspace(B: int, S: int, device) -> torch.Tensor:
    return torch.empty(B * (-(-S * S // SEGLOSS_CHUNK)) * 8, device=device, dtype=torch.float64)


def seg_loss(probs, mask, *, sums=None, loss=None, workspace=None):
    """FocalLoss() + the two BinaryDiceLoss() of forward_utils.py:219-227. probs [B, 2, S, S],
    mask [B, S, S] fp32 in [0, 1] -> (sums [B, 8] fp64, loss [4] fp32 = focal, dice0, dice1, total)."""
    _dev(probs, mask, sums, loss, workspace)
    if probs.dim() != 4 or probs.shape[1] != 2 or probs.shape[2] != probs.shape[3]:
        raise ValueError("probs must be [B, 2, S, S]")
    B, _, S, _ = probs.shape
    _f32c(probs, "probs")
    _f32c(mask, "mask", (B, S, S))
    if sums is None:
        sums = torch.empty(B, 8, device=probs.device, dtype=torch.float64)
    if loss is None:
        loss = torch.empty(4, device=probs.device, dtype=torch.float32)
    if workspace is None:
        workspace = seg_loss_workspace(B, S, probs.device)
    if sums.dtype != torch.float64 or tuple(sums.shape) != (B, 8) or not sums.is_contiguous():
        raise ValueError("sums must be contiguous fp64 [B, 8]")
    if workspace.dtype != torch.float64 or not workspace.is_contiguous():
        raise ValueError("seg_loss workspace must be contiguous fp64")
    _f32c(loss, "loss", (4,))
    _launch("segloss", "seg_loss", 0.0, 3.0 * B * S * S * 4, "aaclip_seg_loss", _ptr(probs), _ptr(mask), B, S,
            _ptr(workspace), workspace.numel() * 8, _ptr(sums), _ptr(loss), _stream())
    return sums, loss


def seg_loss_bwd(probs, mask, sums, dloss, dprobs=None):
    """dprobs [B, 2, S, S] = dloss * d total / d probs; dloss is a device fp32 scalar."""
    _dev(probs, mask, sums, dloss, dprobs)
    if probs.dim() != 4 or probs.shape[1] != 2 or probs.shape[2] != probs.shape[3]:
        raise ValueError("probs must be [B, 2, S, S]")
    B, _, S, _ = probs.shape
    _f32c(probs, "probs")
    _f32c(mask, "mask", (B, S, S))
    if sums.dtype != torch.float64 or tuple(sums.shape) != (B, 8) or not sums.is_contiguous():
        raise ValueError("sums must be contiguous fp64 [B, 8]")
    if dloss.dtype != torch.float32 or dloss.numel() != 1:
        raise ValueError("dloss must be one fp32 device scalar")
    if dprobs is None:
        dprobs = torch.empty_like(probs)
    _f32c(dprobs, "dprobs", probs.shape)
    _launch("segloss", "seg_loss_bwd", 0.0, 5.0 * B * S * S * 4, "aaclip_seg_loss_bwd", _ptr(probs), _ptr(mask),
            _ptr(sums), _ptr(dloss), B, S, _ptr(dprobs), _stream())
    return dprobs


def upsample_softmax_bwd(grid, dprobs, dgrid=None):
    """Backward of blur_upsample(ksize=0, softmax=True) for two channels: grid [B, 2, g, g]
    (the logits the forward took), dprobs [B, 2, S, S] -> dgrid [B, 2, g, g]."""
    _dev(grid, dprobs, dgrid)
    if grid.dim() != 4 or grid.shape[2] != grid.shape[3] or dprobs.dim() != 4 or dprobs.shape[2] != dprobs.shape[3]:
        raise ValueError("upsample_softmax_bwd takes grid [B, 2, g, g] and dprobs [B, 2, S, S]")
    B, C, g, _ = grid.shape
    S = dprobs.shape[-1]
    if C != 2:
        raise ValueError(f"upsample_softmax_bwd supports 2 channels, got {C}")
    _f32c(grid, "grid")
    _f32c(dprobs, "dprobs", (B, C, S, S))
    if dgrid is None:
        dgrid = torch.empty_like(grid)
    _f32c(dgrid, "dgrid", grid.shape)
    _launch("segloss", "upsample_softmax_bwd", 0.0, (2.0 * B * S * S + 4.0 * B * g * g) * 4,
            "aaclip_upsample_softmax_bwd", _ptr(grid), _ptr(dprobs), B, C, g, S, _ptr(dgrid), _stream())
    return dgrid


def patch_logits_bwd_workspace(rows: int, group: int, device) -> torch.Tensor:
    nbytes = ctypes.c_size_t(0)
    call("aaclip_patch_logits_bwd_workspace", rows, group, ctypes.byref(nbytes))
    return torch.empty(int(nbytes.value) // 4, device=device, dtype=torch.float32)


def patch_logits_bwd(f, T, dgrid, *, group, need_dT=True, need_df=True, workspace=None):
    """Backward of the two-anchor train logits: returns (dT, df), None for the one not asked for.
    dT has T's shape ([C, 2] shared: summed over the images; [B, C, 2] per image), df is fp32 [rows, C]."""
    _dev(f, T, dgrid, workspace)
    _rowmajor(f, "f")
    rows, C = f.shape
    if group <= 0 or rows % group:
        raise ValueError("group = patches per image must divide the rows")
    if not (need_dT or need_df):
        raise ValueError("patch_logits_bwd: ask for dT, df or both")
    B = rows // group
    t_stride, _ = _anchors(T, C, B, n_anchor=2)
    if dgrid.numel() != rows * 2:
        raise ValueError("dgrid must be [B, 2, group]")
    _f32c(dgrid, "dgrid")
    dT = torch.empty_like(T) if need_dT else None
    df = torch.empty(rows, C, device=f.device, dtype=torch.float32) if need_df else None
    if need_dT and workspace is None:
        workspace = patch_logits_bwd_workspace(rows, group, f.device)
    if workspace is not None and (workspace.dtype != torch.float32 or not workspace.is_contiguous()):
        raise ValueError("patch_logits_bwd workspace must be contiguous fp32")
    nb = (rows * C * f.element_size() if need_dT else 0) + (rows * C * 4 if need_df else 0) + rows * 2 * 4
    _launch("segloss", "patch_logits_bwd", 4.0 * rows * C * (int(need_dT) + int(need_df)), nb,
            "aaclip_patch_logits_bwd", dtag(f), _ptr(f), f.stride(0), _ptr(T), t_stride, 2, _ptr(dgrid), rows, C,
            group, _ptr(workspace), 0 if workspace is None else workspace.numel() * 4, _ptr(dT), _ptr(df), _stream())
    return dT, df


# ------------------------------------------------------------------------ text-tower backward
WGRAD_ROWS = 64     # AACLIP_WGRAD_ROWS
ATTN_BWD_MAX_SEQ = 77
_ACT_MODES = {"gelu": _lib.EPI_GELU, True: _lib.EPI_GELU, "quick": _lib.EPI_QGELU, "leaky": _lib.EPI_LEAKY}


def _f32rows(t, name, shape=None):
    """fp32, 2-D, unit column stride, 16-byte aligned rows (the row kernels move float4)."""
    _rowmajor(t, name)
    if t.dtype != torch.float32 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name} must be fp32" + (f" {list(shape)}" if shape is not None else ""))
    if t.stride(0) % 4 or t.data_ptr() % 16:
        raise ValueError(f"{name}: row stride must be a multiple of 4 and the start 16-byte aligned")


def _overlap(a, b) -> bool:
    """Whether a and b share a byte. A 2-D tensor with unit column stride is its rows (exact when the
    two row strides agree or one side is a single row: column views of one buffer do not overlap);
    anything else must be contiguous and is one range. Two different row strides whose ranges meet
    count as overlapping."""
    def rows(t):
        if t.dim() == 2 and t.stride(1) == 1 and t.shape[0] > 1:
            return t.data_ptr(), t.shape[0], t.stride(0) * t.element_size(), t.shape[1] * t.element_size()
        return t.data_ptr(), 1, 0, t.numel() * t.element_size()

    (pa, ra, sa, wa), (pb, rb, sb, wb) = rows(a), rows(b)
    if min(wa, wb) == 0 or pa + (ra - 1) * sa + wa <= pb or pb + (rb - 1) * sb + wb <= pa:
        return False
    s = sa if ra > 1 else sb
    if s == 0 or (ra > 1 and rb > 1 and sa != sb):
        return True
    d = pb - pa  # row i of a meets row j of b iff -wb < d + (j - i) s < wa
    return max(-(ra - 1), (-wb - d) // s + 1) <= min(rb - 1, -((d - wa) // s) - 1)


def _same_view(a, b) -> bool:
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def _disjoint(op, out, out_name, *inputs, may_be=()):
    """out must share no memory with any of the (tensor, name) inputs; the tensors of may_be may
    instead be out itself, element for element (the kernels read a row before they write it)."""
    for t, name in inputs:
        if t is not None and _overlap(out, t) and not (any(t is m for m in may_be) and _same_view(out, t)):
            raise ValueError(f"{op}: {out_name} overlaps {name}" +
                             (" without being the same view" if any(t is m for m in may_be) else ""))


def _act_mode(mode):
    try:
        return _ACT_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("activation mode must be 'gelu' (or True), 'quick' or 'leaky'") from None


def attention_bwd(qkv, dout, batch: int, seq: int, heads: int, *, causal: bool = False, dqkv=None):
    """dqkv [batch*seq, 3*heads*64] of the fp32 attention core from its packed qkv and dout
    [batch*seq, heads*64]; seq <= 77 (the text context)."""
    hd = 64
    if not 1 <= seq <= ATTN_BWD_MAX_SEQ:
        raise ValueError(f"attention_bwd holds one sequence in LDS: seq must be 1..{ATTN_BWD_MAX_SEQ}, got {seq}")
    if batch < 1 or heads < 1:
        raise ValueError("attention_bwd needs batch >= 1 and heads >= 1")
    _f32c(qkv, "qkv", (batch * seq, 3 * heads * hd))
    _f32c(dout, "dout", (batch * seq, heads * hd))
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    _f32c(dqkv, "dqkv", qkv.shape)
    if dqkv.data_ptr() == qkv.data_ptr():
        raise ValueError("attention_bwd: dqkv must not alias qkv")
    _dev(qkv, dout, dqkv)  # after the shape / dtype checks: those need no device
    _launch("text_bwd", "attention_bwd", 10.0 * batch * heads * seq * seq * hd / (2 if causal else 1),
            (2 * qkv.numel() + dout.numel()) * 4, "aaclip_attention_bwd", _ptr(qkv), _ptr(dout), _ptr(dqkv), batch,
            seq, heads, hd, _lib.ATTN_CAUSAL if causal else 0, _stream())
    return dqkv


def layernorm_bwd(dy, x, w, *, residual=None, out=None):
    """out = [residual +] LN_bwd(dy; x, w) per row (no dw / db); residual and dy may be out."""
    _f32rows(x, "x")
    rows, width = x.shape
    if width not in (768, 1024):
        raise ValueError("layernorm_bwd supports widths 768 and 1024")
    _f32rows(dy, "dy", x.shape)
    if w.dtype != torch.float32 or tuple(w.shape) != (width,) or not w.is_contiguous() or w.data_ptr() % 16:
        raise ValueError("w must be contiguous fp32 [width]")
    if residual is not None:
        _f32rows(residual, "residual", x.shape)
    if out is None:
        out = torch.empty(rows, width, device=x.device, dtype=torch.float32)
    _f32rows(out, "out", x.shape)
    _disjoint("layernorm_bwd", out, "out", (x, "x"), (dy, "dy"), (residual, "residual"), may_be=(dy, residual))
    _dev(dy, x, w, residual, out)  # after the shape / dtype checks: those need no device
    _launch("text_bwd", "layernorm_bwd", 0.0, rows * width * 4 * (4 if residual is not None else 3),
            "aaclip_layernorm_bwd", _ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(w), _ptr(residual),
            0 if residual is None else residual.stride(0), _ptr(out), out.stride(0), rows, width, _stream())
    return out


def eot_ln_bwd(dy, x, tokens, w, *, out=None):
    """g [n*ctx, width]: the ln_final backward of dy [n, width] at each sequence's EOT row, 0 elsewhere."""
    if tokens.dim() != 2 or tokens.dtype != torch.int32 or not tokens.is_contiguous():
        raise ValueError("tokens must be contiguous int32 [n, ctx]")
    n, ctx = tokens.shape
    if n < 1 or ctx < 1:
        raise ValueError("eot_ln_bwd needs at least one sequence and one token")
    if x.dim() != 2 or x.shape[0] != n * ctx or x.shape[1] not in (768, 1024):
        raise ValueError("x must be [n*ctx, width] with width 768 or 1024")
    width = x.shape[1]
    _f32c(x, "x")
    _f32c(dy, "dy", (n, width))
    _f32c(w, "w", (width,))
    if out is None:
        out = torch.empty_like(x)
    _f32c(out, "out", x.shape)
    _disjoint("eot_ln_bwd", out, "out", (x, "x"), (dy, "dy"))
    for t, nm in ((x, "x"), (dy, "dy"), (w, "w"), (out, "out")):
        if t.data_ptr() % 16:
            raise ValueError(f"eot_ln_bwd: {nm} must be 16-byte aligned")
    _dev(dy, x, tokens, w, out)  # after the shape / dtype checks: those need no device
    _launch("text_bwd", "eot_ln_bwd", 0.0, (x.numel() + 2 * n * width) * 4, "aaclip_eot_ln_bwd", _ptr(dy), _ptr(x),
            _ptr(tokens), _ptr(w), _ptr(out), n, ctx, width, _stream())
    return out


def act(x, mode, *, out=None):
    """out = f(x), f = the fp32 GEMM epilogue's own 'gelu' / 'quick' / 'leaky' (out may be x)."""
    m = _act_mode(mode)
    _f32c(x, "x")
    if out is None:
        out = torch.empty_like(x)
    _f32c(out, "out", x.shape)
    _dev(x, out)  # after the shape / dtype checks: those need no device
    _launch("text_bwd", "act", 0.0, 8.0 * x.numel(), "aaclip_act", m, _ptr(x), _ptr(out), x.numel(), _stream())
    return out


def act_bwd(dy, ref, mode, *, out=None):
    """out = dy * f'(.): ref is the pre-activation for 'gelu' / 'quick', the OUTPUT for 'leaky'."""
    m = _act_mode(mode)
    _f32c(dy, "dy")
    _f32c(ref, "ref", dy.shape)
    if out is None:
        out = torch.empty_like(dy)
    _f32c(out, "out", dy.shape)
    _dev(dy, ref, out)  # after the shape / dtype checks: those need no device
    _launch("text_bwd", "act_bwd", 0.0, 12.0 * dy.numel(), "aaclip_act_bwd", m, _ptr(dy), _ptr(ref), _ptr(out),
            dy.numel(), _stream())
    return out


def adapter_blend_bwd(dy, x, u, adapt_weight: float, *, dx=None, du=None):
    """(dx, du) of y = w u |x| / |u| + (1 - w) x; dx is the path through x alone and may be dy."""
    if x.dim() != 2 or x.shape[1] not in (768, 1024):
        raise ValueError("adapter_blend_bwd takes [rows, 768 | 1024] tensors")
    _f32c(x, "x")
    _f32c(dy, "dy", x.shape)
    _f32c(u, "u", x.shape)
    if dx is None:
        dx = torch.empty_like(x)
    if du is None:
        du = torch.empty_like(x)
    _f32c(dx, "dx", x.shape)
    _f32c(du, "du", x.shape)
    _disjoint("adapter_blend_bwd", dx, "dx", (x, "x"), (u, "u"), (dy, "dy"), may_be=(dy,))  # dx alone may be dy
    _disjoint("adapter_blend_bwd", du, "du", (x, "x"), (u, "u"), (dy, "dy"), (dx, "dx"))
    for t in (dy, x, u, dx, du):
        if t.data_ptr() % 16:
            raise ValueError("adapter_blend_bwd operands must be 16-byte aligned")
    _dev(dy, x, u, dx, du)  # after the shape / dtype checks: those need no device
    _launch("text_bwd", "adapter_blend_bwd", 0.0, 20.0 * x.numel(), "aaclip_adapter_blend_bwd", _ptr(dy), _ptr(x),
            _ptr(u), float(adapt_weight), _ptr(dx), _ptr(du), x.shape[0], x.shape[1], _stream())
    return dx, du


def anchor_reduce_bwd(emb, dT, col: int, *, out=None):
    """demb [n, dim] from dT[:, col] through normalize(mean_s normalize(emb[s]))."""
    if emb.dim() != 2 or not 1 <= emb.shape[0] <= 256 or not 1 <= emb.shape[1] <= 1024:
        raise ValueError("emb must be [n <= 256, dim <= 1024]")
    _f32c(emb, "emb")
    n, dim = emb.shape
    if dT.dim() != 2 or dT.shape[0] != dim or not 0 <= col < dT.shape[1]:
        raise ValueError("dT must be [dim, ncols] with 0 <= col < ncols")
    _f32c(dT, "dT")
    if out is None:
        out = torch.empty_like(emb)
    _f32c(out, "out", emb.shape)
    _disjoint("anchor_reduce_bwd", out, "out", (emb, "emb"))
    _dev(emb, dT, out)  # after the shape / dtype checks: those need no device
    _launch("text_bwd", "anchor_reduce_bwd", 0.0, 16.0 * emb.numel(), "aaclip_anchor_reduce_bwd", _ptr(emb), n, dim,
            _ptr(dT), col, dT.shape[1], _ptr(out), _stream())
    return out


def linear_wgrad_workspace(M: int, N: int, K: int, device) -> torch.Tensor:
    nbytes = ctypes.c_size_t(0)
    call("aaclip_linear_wgrad_workspace", M, N, K, ctypes.byref(nbytes))
    return torch.empty(int(nbytes.value) // 4, device=device, dtype=torch.float32)


def linear_wgrad(dy, x, *, out=None, workspace=None):
    """dW [N, K] = dy[M, N]^T x[M, K], the weight gradient of a bias-free Linear (N, K % 64 == 0)."""
    _rowmajor(dy, "dy")
    _rowmajor(x, "x")
    if dy.dtype != torch.float32 or x.dtype != torch.float32:
        raise ValueError("linear_wgrad takes fp32 operands")
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M or M < 1 or N % 64 or K % 64 or N < 64 or K < 64:
        raise ValueError(f"linear_wgrad: dy [M, N] and x [M, K] with M >= 1, N and K multiples of 64; got "
                         f"{tuple(dy.shape)} {tuple(x.shape)}")
    if out is None:
        out = torch.empty(N, K, device=dy.device, dtype=torch.float32)
    _rowmajor(out, "out")
    if out.dtype != torch.float32 or tuple(out.shape) != (N, K):
        raise ValueError("linear_wgrad: out must be fp32 [N, K]")
    if workspace is None:
        workspace = linear_wgrad_workspace(M, N, K, dy.device)
    if workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise ValueError("linear_wgrad workspace must be contiguous fp32")
    _disjoint("linear_wgrad", out, "out", (dy, "dy"), (x, "x"), (workspace, "workspace"))
    _disjoint("linear_wgrad", workspace, "workspace", (dy, "dy"), (x, "x"))
    _dev(dy, x, out, workspace)  # after the shape / dtype checks: those need no device
    _launch("text_bwd", "linear_wgrad", 2.0 * M * N * K, (M * (N + K) + 2 * N * K) * 4, "aaclip_linear_wgrad",
            _ptr(dy), dy.stride(0), _ptr(x), x.stride(0), M, N, K, _ptr(workspace), workspace.numel() * 4, _ptr(out),
            out.stride(0), _stream())
    return out


# ------------------------------------------------------------------------ stage-2 backward
def _attention_bwd_workspace(entry: str, batch: int, seq: int, heads: int, device) -> torch.Tensor:
    nbytes = ctypes.c_size_t(0)
    call(f"aaclip_{entry}_workspace", batch, seq, heads, ctypes.byref(nbytes))
    return torch.empty(int(nbytes.value) // 4, device=device, dtype=torch.float32)


def _attention_bwd(entry: str, dtype, lead: tuple, flags: tuple, qkv, out, dout, batch: int, seq: int, heads: int,
                   dqkv, workspace):
    """The tiled attention backward behind attention_bwd_tiled (fp32) and attention_bwd16 (bf16):
    `dtype` is the operands' element type, `lead` / `flags` the entry's arguments before qkv /
    after head_dim."""
    def check(t, name, shape):
        if dtype == torch.float32:
            _f32c(t, name, shape)
        else:
            _c16(t, name, dtype, shape)

    hd = 64
    if batch < 1 or heads < 1 or seq < 1:
        raise ValueError(f"{entry} needs batch, heads and seq >= 1")
    if batch * heads > 65535:
        raise ValueError(f"{entry}: batch * heads must be <= 65535")
    check(qkv, "qkv", (batch * seq, 3 * heads * hd))
    check(out, "out", (batch * seq, heads * hd))
    check(dout, "dout", (batch * seq, heads * hd))
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    check(dqkv, "dqkv", qkv.shape)
    if dqkv.data_ptr() in (qkv.data_ptr(), out.data_ptr(), dout.data_ptr()):
        raise ValueError(f"{entry}: dqkv must not alias qkv, out or dout")
    if workspace is None:
        workspace = _attention_bwd_workspace(entry, batch, seq, heads, qkv.device)
    if workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise ValueError(f"{entry} workspace must be contiguous fp32")
    for t in (qkv, out, dout, dqkv, workspace):
        if t.data_ptr() % 16:
            raise ValueError(f"{entry} operands must be 16-byte aligned")
    _dev(qkv, out, dout, dqkv, workspace)  # after the shape / dtype checks: those need no device
    # 2 launches: S twice + dP + dQ, and S + dP + dV + dK: 16 seq^2 hd FLOPs per (image, head)
    _launch("visual_bwd", entry, 16.0 * batch * heads * seq * seq * hd,
            (3 * qkv.numel() + 3 * dout.numel()) * qkv.element_size(), f"aaclip_{entry}", *lead, _ptr(qkv), _ptr(out),
            _ptr(dout), _ptr(dqkv), batch, seq, heads, hd, *flags, _ptr(workspace), workspace.numel() * 4, _stream())
    return dqkv


def attention_bwd_tiled_workspace(batch: int, seq: int, heads: int, device) -> torch.Tensor:
    return _attention_bwd_workspace("attention_bwd_tiled", batch, seq, heads, device)


def attention_bwd_tiled(qkv, out, dout, batch: int, seq: int, heads: int, *, dqkv=None, workspace=None):
    """dqkv [batch*seq, 3*heads*64] of the fp32 non-causal attention core, any seq >= 1, from
    the packed qkv, the forward's output out and dout (both [batch*seq, heads*64])."""
    return _attention_bwd("attention_bwd_tiled", torch.float32, (), (), qkv, out, dout, batch, seq, heads, dqkv,
                          workspace)


def tap_ln_bwd(dtap, x, w, g, batch: int, n_tok: int):
    """g[b, t] += LN_bwd(dtap[b, t - 1]; x[b, t], w) for the token rows t >= 1 (in place; CLS rows
    of g untouched): the backward of block_tail's level tap through ln_post."""
    if x.dim() != 2 or x.shape[1] not in (768, 1024) or batch < 1 or n_tok < 2 or x.shape[0] != batch * n_tok:
        raise ValueError("x must be [batch*n_tok, 768 | 1024] with n_tok >= 2")
    width = x.shape[1]
    _f32c(x, "x")
    _f32c(g, "g", x.shape)
    _f32c(dtap, "dtap", (batch * (n_tok - 1), width))
    _f32c(w, "w", (width,))
    _disjoint("tap_ln_bwd", g, "g", (x, "x"), (dtap, "dtap"))
    for t in (dtap, x, w, g):
        if t.data_ptr() % 16:
            raise ValueError("tap_ln_bwd operands must be 16-byte aligned")
    _dev(dtap, x, w, g)  # after the shape / dtype checks: those need no device
    _launch("visual_bwd", "tap_ln_bwd", 0.0, 16.0 * x.numel(), "aaclip_tap_ln_bwd", _ptr(dtap), _ptr(x), _ptr(w),
            _ptr(g), batch, n_tok, width, _stream())
    return g


def l2_normalize_bwd(dy, x, *, group: int = 0, scale: float = 1.0, out=None):
    """dx of y = x / max(|x|, 1e-12) per row of x [rows, 768 | 1024]. group == 0: dy is
    [rows, width]; group > 0: row r takes scale * dy[r // group] (dy [rows / group, width]),
    the backward of normalize(x).view(-1, group, width).mean(1) with scale = 1 / group."""
    _f32rows(x, "x")
    rows, width = x.shape
    if width not in (768, 1024):
        raise ValueError("l2_normalize_bwd supports widths 768 and 1024")
    if group < 0 or (group > 0 and rows % group):
        raise ValueError("l2_normalize_bwd: rows must be a multiple of group")
    _f32rows(dy, "dy", (rows // group if group else rows, width))
    if out is None:
        out = torch.empty(rows, width, device=x.device, dtype=torch.float32)
    _f32rows(out, "out", x.shape)
    # out may be dy only row for row: never under a group
    _disjoint("l2_normalize_bwd", out, "out", (x, "x"), (dy, "dy"), may_be=() if group else (dy,))
    _dev(dy, x, out)  # after the shape / dtype checks: those need no device
    _launch("visual_bwd", "l2_normalize_bwd", 0.0, 12.0 * rows * width, "aaclip_l2_normalize_bwd", _ptr(dy),
            dy.stride(0), int(group), float(scale), _ptr(x), x.stride(0), _ptr(out), out.stride(0), rows, width,
            _stream())
    return out


# ------------------------------------------------------------------------ stage-2 backward, bf16
_H16 = (torch.bfloat16, torch.float16)


def _c16(t, name, dtype, shape=None):
    if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name} must be contiguous {dtype}" + (f" {list(shape)}" if shape is not None else ""))


def attention_bwd16_workspace(batch: int, seq: int, heads: int, device) -> torch.Tensor:
    return _attention_bwd_workspace("attention_bwd16", batch, seq, heads, device)


def attention_bwd16(qkv, out, dout, batch: int, seq: int, heads: int, *, q_prescaled: bool = False, dqkv=None,
                    workspace=None):
    """bf16 dqkv [batch*seq, 3*heads*64] of the bf16 non-causal attention core, any seq >= 1, from
    the packed bf16 qkv, the forward's bf16 output out and bf16 dout (both [batch*seq, heads*64]).
    q_prescaled: the q columns carry log2(e)/sqrt(64) (ops.attention's flag); the q columns of
    dqkv are then the gradient of that prescaled q."""
    return _attention_bwd("attention_bwd16", torch.bfloat16, (_lib.BF16,),
                          (_lib.ATTN_Q_PRESCALED if q_prescaled else 0,), qkv, out, dout, batch, seq, heads, dqkv,
                          workspace)


def act_to16(x, mode, *, out):
    """out (contiguous bf16 / fp16, x's shape) = f(x) of fp32 x with the 16-bit GEMM epilogue's own
    'gelu' / 'quick' / 'leaky' and rounding."""
    m = _act_mode(mode)
    _f32c(x, "x")
    if out.dtype not in _H16:
        raise ValueError("act_to16: out must be bfloat16 or float16")
    _c16(out, "out", out.dtype, x.shape)
    if x.data_ptr() % 16 or out.data_ptr() % 16:
        raise ValueError("act_to16 operands must be 16-byte aligned")
    _dev(x, out)  # after the shape / dtype checks: those need no device
    _launch("visual_bwd", "act_to16", 0.0, 6.0 * x.numel(), "aaclip_act_to16", m, _ptr(x), _ptr(out), dtag(out),
            x.numel(), _stream())
    return out


def act_bwd16(dy, ref, mode, *, out=None):
    """out = round(dy * f'(.)) with 16-bit dy / out and the fp32 reference value (ops.act_bwd's: the
    pre-activation for 'gelu' / 'quick', the output for 'leaky'); out may be dy."""
    m = _act_mode(mode)
    if dy.dtype not in _H16:
        raise ValueError("act_bwd16: dy must be bfloat16 or float16")
    _c16(dy, "dy", dy.dtype)
    _f32c(ref, "ref", dy.shape)
    if out is None:
        out = torch.empty_like(dy)
    _c16(out, "out", dy.dtype, dy.shape)
    for t in (dy, ref, out):
        if t.data_ptr() % 16:
            raise ValueError("act_bwd16 operands must be 16-byte aligned")
    _dev(dy, ref, out)  # after the shape / dtype checks: those need no device
    _launch("visual_bwd", "act_bwd16", 0.0, 8.0 * dy.numel(), "aaclip_act_bwd16", m, _ptr(dy), _ptr(ref), _ptr(out),
            dtag(dy), dy.numel(), _stream())
    return out


def cast_rows(x, out=None, *, dtype=None):
    """out = x in the other precision, row by row: fp32 -> bf16 / fp16 (round to nearest even, the GEMM
    epilogue's conversion) or bf16 / fp16 -> fp32 (exact). 2-D, unit column stride, columns a
    multiple of 8, 16-byte aligned rows; out (or a fresh contiguous tensor of `dtype`) is returned."""
    _rowmajor(x, "x")
    if out is None:
        if dtype is None:
            raise ValueError("cast_rows needs out or dtype")
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    _rowmajor(out, "out")
    pair = (x.dtype, out.dtype)
    if not ((pair[0] == torch.float32 and pair[1] in _H16) or (pair[0] in _H16 and pair[1] == torch.float32)):
        raise ValueError("cast_rows converts float32 -> bfloat16 / float16 or bfloat16 / float16 -> float32")
    if tuple(out.shape) != tuple(x.shape) or x.shape[1] % 8 or x.shape[1] == 0:
        raise ValueError("cast_rows: out must have x's shape and the columns must be a multiple of 8")
    for t in (x, out):
        if (t.stride(0) * t.element_size()) % 16 or t.data_ptr() % 16 or t.stride(0) < t.shape[1]:
            raise ValueError("cast_rows: rows must be 16-byte aligned")
    if x.data_ptr() == out.data_ptr():
        raise ValueError("cast_rows: out must not alias x")
    _dev(x, out)  # after the shape / dtype checks: those need no device
    _launch("visual_bwd", "cast_rows", 0.0, 6.0 * x.numel(), "aaclip_cast_rows", dtag(x), dtag(out), _ptr(x),
            x.stride(0), _ptr(out), out.stride(0), x.shape[0], x.shape[1], _stream())
    return out


class _AnchorColumn(torch.autograd.Function):
    """One anchor column normalize(mean_s normalize(emb[s])) with a backward to emb."""

    @staticmethod
    def forward(ctx, emb_in, emb):
        T = torch.empty(emb.shape[1], 1, device=emb.device, dtype=torch.float32)
        anchor_reduce(emb, T, 0)
        ctx.save_for_backward(emb)
        ctx.meta = (emb_in.shape, emb_in.dtype, emb_in.device)
        return T[:, 0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dt):
        (emb,) = ctx.saved_tensors
        with torch.cuda.device(emb.device):
            dT = dt.to(emb.device, torch.float32).reshape(-1, 1).contiguous()
            demb = anchor_reduce_bwd(emb, dT, 0)
        return demb.reshape(ctx.meta[0]).to(device=ctx.meta[2], dtype=ctx.meta[1]), None


def anchor_column(emb: torch.Tensor) -> torch.Tensor:
    """[dim] = normalize(mean_s normalize(emb[s])) (aaclip_anchor_reduce, the bits anchor_reduce
    writes into a T column). When emb carries grad the result does too (aaclip_anchor_reduce_bwd)."""
    _dev(emb)
    e = emb.detach().to(torch.float32).contiguous()
    if torch.is_grad_enabled() and emb.requires_grad:
        with torch.cuda.device(e.device):
            return _AnchorColumn.apply(emb, e)
    T = torch.empty(e.shape[1], 1, device=e.device, dtype=torch.float32)
    anchor_reduce(e, T, 0)
    return T[:, 0]


def anomaly_map(levels, T, out, grid_ws, *, g, ksize, sigma, normalize=True):
    """Test-branch map of all levels: patch_scores into grid_ws (>= B*g*g fp32), then blur_upsample."""
    _dev(*levels, T, out, grid_ws)
    B, S, S2 = out.shape
    rows, C = levels[0].shape
    if rows != B * g * g or S != S2 or grid_ws.numel() < rows or grid_ws.dtype != torch.float32:
        raise ValueError("anomaly_map shape mismatch (grid_ws: fp32 >= [B*g*g])")
    if not out.is_contiguous():
        raise ValueError("anomaly_map output must be contiguous")
    for t in levels:
        if t.shape != (rows, C) or t.stride(0) != levels[0].stride(0) or t.dtype != levels[0].dtype:
            raise ValueError("levels must share shape, dtype and stride")
    arr = _level_array(levels)
    nb = len(levels) * rows * C * levels[0].element_size() + C * 2 * 4 + B * S * S * 4 + 2 * rows * 4
    _launch("anomaly_map", "anomaly_map (patch_scores + blur_upsample)", 0.0, nb, "aaclip_anomaly_map",
            dtag(levels[0]), arr, len(levels), levels[0].stride(0), _ptr(T), B, g, C, int(normalize), S, ksize,
            float(sigma), _ptr(grid_ws), _ptr(out), _stream())
    return out


SCORE_GROUPS = 768 // 32  # float4 partials per (row, level) written by gemm_scores


def gemm_scores(a: torch.Tensor, w: torch.Tensor, T: torch.Tensor, part: torch.Tensor, *, leaky=False):
    """Level projection straight into anomaly-map partials (aaclip_gemm_scores): for
    v = LeakyReLU?(a @ w.T), part[m, 4g:4g+4] = {||v||^2, v.t0, v.t1, 0} over columns
    32g..32g+31, t = T[c % 768]. part: fp32 view [M, >= N/8] (unit column stride)."""
    _dev(a, w, T, part)
    _rowmajor(a, "a")
    _rowmajor(w, "w")
    _rowmajor(part, "part")
    if a.dtype not in (torch.bfloat16, torch.float16) or w.dtype != a.dtype:
        raise TypeError("gemm_scores: 16-bit operands of one dtype")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or part.shape[0] != M or part.shape[1] < N // 8 or part.dtype != torch.float32:
        raise ValueError("gemm_scores shape mismatch")
    if T.dtype != torch.float32 or not T.is_contiguous() or T.shape != (768, 2):
        raise ValueError("gemm_scores: T must be contiguous fp32 [768, 2]")
    _launch(f"gemm N{N} K{K} scores" + (" leaky" if leaky else ""), lambda: gemm_plan(dtag(a), M, N, K),
            2.0 * M * N * K, (M * K + N * K) * a.element_size() + M * N // 8 * 4, "aaclip_gemm_scores", dtag(a), M,
            N, K, _ptr(a), a.stride(0), _ptr(w), w.stride(0), 4 if leaky else 0, _ptr(T), 768, _ptr(part),
            part.stride(0), _stream())


def anomaly_map_partials(part, n_levels, out, grid_ws, *, g, ksize, sigma, det_ws=None, score=None):
    """Map (+ image score when det_ws / score are given) from gemm_scores partials
    (aaclip_anomaly_map_partials): part [B*g*g, >= (n_levels + det) * 96] fp32."""
    _dev(part, out, grid_ws, det_ws, score)
    _rowmajor(part, "part")
    B, S, S2 = out.shape
    rows = B * g * g
    det = det_ws is not None
    if part.shape[0] != rows or part.shape[1] < (n_levels + det) * 4 * SCORE_GROUPS or S != S2:
        raise ValueError("anomaly_map_partials shape mismatch")
    if grid_ws.numel() < rows or (det and (det_ws.numel() < rows or score is None or score.numel() < B)):
        raise ValueError("anomaly_map_partials workspace too small")
    if not out.is_contiguous():
        raise ValueError("anomaly_map_partials output must be contiguous")
    nb = rows * (n_levels + det) * 4 * SCORE_GROUPS * 4 + B * S * S * 4 + 2 * rows * 4
    _launch("anomaly_map", "anomaly_map (partial_scores + blur_upsample)", 0.0, nb, "aaclip_anomaly_map_partials",
            _ptr(part), part.stride(0), n_levels, int(det), B, g, S, ksize, float(sigma), _ptr(grid_ws),
            _ptr(det_ws), _ptr(out), _ptr(score), _stream())
    return out


def image_score(det_raw, batch, n_patch, partial, det=None, T=None, score=None, normalize=True):
    _dev(det_raw, partial, det, T, score)
    _rowmajor(det_raw, "det_raw")
    rows, C = det_raw.shape
    if rows != batch * n_patch or partial.numel() < batch * ((n_patch + 15) // 16) * C:
        raise ValueError("image_score shape mismatch")
    _launch("image_score", "image_score (det_partial + det_finalize)", 0.0, rows * C * det_raw.element_size(),
            "aaclip_image_score", dtag(det_raw), _ptr(det_raw), det_raw.stride(0), _ptr(T), batch, n_patch, C,
            int(normalize), _ptr(partial), _ptr(det), _ptr(score), _stream())


def _pro_hw(pixel_preds, pixel_label):
    """(H, W) of [n, H, W] / [n, 1, H, W] pixel tensors: the components need the image shape."""
    def hw(t, name):
        if t.dim() == 4 and t.shape[1] == 1:
            return tuple(t.shape[2:])
        if t.dim() == 3:
            return tuple(t.shape[1:])
        raise ValueError(f"pro=True needs {name} as [n, H, W] or [n, 1, H, W], got {tuple(t.shape)}")
    a, b = hw(pixel_preds, "pixel_preds"), hw(pixel_label, "pixel_label")
    if a != b:
        raise ValueError(f"pixel_preds and pixel_label must have the same image shape, got {a} and {b}")
    return a


def _metrics_operands(pixel_preds, pixel_label, image_preds, image_label):
    N = pixel_preds.shape[0]
    preds = pixel_preds.reshape(N, -1).to(torch.float32).contiguous()
    lab = pixel_label.reshape(N, -1)
    if lab.shape[1] != preds.shape[1]:
        raise ValueError("pixel_label and pixel_preds must have the same number of elements per image")
    lab = (lab != 0).to(torch.uint8).contiguous()
    ip = image_preds.reshape(-1).to(torch.float32).contiguous()
    il = (image_label.reshape(-1) != 0).to(torch.uint8).contiguous()
    if ip.numel() != N or il.numel() != N:
        raise ValueError("image_preds / image_label must have one entry per image")
    return N, preds, lab, ip, il


def metrics_eval(pixel_preds: torch.Tensor, pixel_label: torch.Tensor, image_preds: torch.Tensor,
                 image_label: torch.Tensor, *, medical: bool, pro: bool = False,
                 fpr_limit: float = 0.3, f1: bool = False) -> list[float]:
    """Device metrics_eval of one class (aaclip_metrics_eval): returns the unrounded
    [pixel AUROC, pixel AP, image AUROC, image AP]. pixel_preds [N, ...] fp32 maps,
    pixel_label same element count (nonzero = anomalous), image_* [N]. With pro=True
    (aaclip_metrics_eval_pro; pixel tensors [N, H, W] or [N, 1, H, W]) a fifth entry follows:
    the pixel AUPRO up to the false-positive rate fpr_limit. With f1=True (aaclip_metrics_eval_f1)
    eight more follow: pixel F1-max, its threshold, precision and recall there, and the same four
    for images; thresholds are in the normalised score domains (see metrics_eval_device)."""
    return metrics_eval_device(pixel_preds, pixel_label, image_preds, image_label, medical=medical, pro=pro,
                               fpr_limit=fpr_limit, f1=f1).tolist()


def metrics_eval_device(pixel_preds, pixel_label, image_preds, image_label, *, medical: bool, pro: bool = False,
                        fpr_limit: float = 0.3, f1: bool = False) -> torch.Tensor:
    """metrics_eval without the host sync: the device float64[4] result, read later (the
    harness reads every class's at the end, so classes are enqueued back to back). With
    pro=True the result is float64[5]: the same four numbers, bit for bit, and the pixel
    AUPRO over the 8-connected components of pixel_label (aaclip_metrics_eval_pro).
    With f1=True (aaclip_metrics_eval_f1) the same 4 (or 5) numbers, bit for bit, are followed by
    pixel F1-max, threshold, precision, recall and image F1-max, threshold, precision, recall:
    float64[12] (or [13]). F1(t) = 2 TP / (PP + P) over the distinct scores t, the threshold the
    lowest maximiser; pixel thresholds are class-normalised map values, image thresholds fused
    image scores, both as the device computes them in fp32. Flattened [N, pix] maps stay legal
    unless pro=True."""
    if pro:
        H, W = _pro_hw(pixel_preds, pixel_label)
        if not 0.0 < float(fpr_limit) <= 1.0:
            raise ValueError(f"fpr_limit must be in (0, 1], got {fpr_limit}")
    N, preds, lab, ip, il = _metrics_operands(pixel_preds, pixel_label, image_preds, image_label)
    with torch.cuda.device(preds.device):
        if f1:
            if not pro:
                H, W = 1, preds.shape[1]  # no labelling: only H * W matters
            out = _metrics_eval_f1_dev(preds, lab, ip, il, N, H, W, medical, pro, float(fpr_limit))
            return out if pro else torch.cat([out[:4], out[5:]])
        if pro:
            return _metrics_eval_pro_dev(preds, lab, ip, il, N, H, W, medical, float(fpr_limit))
        return _metrics_eval_dev(preds, lab, ip, il, N, preds.shape[1], medical)


def _metrics_eval_f1_dev(preds, lab, ip, il, N, H, W, medical, pro, fpr_limit):
    _dev(preds, lab, ip, il)
    need = ctypes.c_size_t(0)
    call("aaclip_metrics_f1_workspace", N * H * W, N, int(pro), ctypes.byref(need))
    ws, at = _aligned_workspace(int(need.value), preds.device)
    out = torch.empty(13, device=preds.device, dtype=torch.float64)
    call("aaclip_metrics_eval_f1", _ptr(preds), _ptr(lab), _ptr(ip), _ptr(il), N, H, W, int(medical), int(pro),
         fpr_limit, at, need.value, _ptr(out), _stream())
    return out


def _aligned_workspace(nbytes, device):
    ws = torch.empty(nbytes + 256, device=device, dtype=torch.uint8)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


def _metrics_eval_pro_dev(preds, lab, ip, il, N, H, W, medical, fpr_limit):
    _dev(preds, lab, ip, il)
    need = ctypes.c_size_t(0)
    call("aaclip_metrics_pro_workspace", N * H * W, N, ctypes.byref(need))
    ws, at = _aligned_workspace(int(need.value), preds.device)
    out = torch.empty(5, device=preds.device, dtype=torch.float64)
    call("aaclip_metrics_eval_pro", _ptr(preds), _ptr(lab), _ptr(ip), _ptr(il), N, H, W, int(medical), fpr_limit,
         at, need.value, _ptr(out), _stream())
    return out


def label_components(mask: torch.Tensor):
    """8-connected components of mask != 0, per image (aaclip_label_components). mask: device
    tensor [n, H, W] or [n, 1, H, W] of any dtype. Returns (labels int64 [n, H, W]: 0 for
    background, else 1 + the smallest linear index y * W + x of the pixel's component; areas
    int64 [n, H, W]: the pixel's component's area; counts int64 [n]: components per image)."""
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dim() != 3 or mask.numel() == 0:
        raise ValueError(f"mask must be a non-empty [n, H, W] or [n, 1, H, W], got {tuple(mask.shape)}")
    m = (mask != 0).to(torch.uint8).contiguous()
    n, H, W = m.shape
    with torch.cuda.device(m.device):
        _dev(m)
        # the C side writes uint32; int32 storage holds the same bits (labels and areas are < 2^31)
        labels = torch.empty(n, H, W, device=m.device, dtype=torch.int32)
        areas = torch.empty(n, H, W, device=m.device, dtype=torch.int32)
        counts = torch.empty(n, device=m.device, dtype=torch.int32)
        call("aaclip_label_components", _ptr(m), n, H, W, _ptr(labels), _ptr(areas), _ptr(counts), _stream())
        return labels.to(torch.int64), areas.to(torch.int64), counts.to(torch.int64) & 0xFFFFFFFF


def extract_regions(pixel_preds, threshold, *, pixel_label=None, normalise=True, min_area=1, max_regions=64):
    """The defect regions of one class's maps (aaclip_extract_regions): the 8-connected components of
    the pixels with v >= threshold, v the class-normalised fp32 map value of the metrics
    (normalise=True: threshold may be the "pixel F1 threshold" of metrics_eval_device(f1=True)) or
    the raw value (normalise=False). pixel_preds: device tensor [n, H, W] or [n, 1, H, W];
    pixel_label: the same shape (nonzero = anomalous) or None. Regions under min_area pixels are
    dropped. Returns device tensors, enqueued without a host sync, as a dict:
      "n_regions" int64 [n]        regions left per image (may exceed max_regions; 0xFFFFFFFF when
                                   the labelling hit a cap)
    and per slot [n, max_regions], an image's regions first, by area descending then label
    ascending, zero past min(n_regions, max_regions):
      "label" int64       1 + the smallest linear index y * W + x of the region
      "area" int64        pixels
      "bbox" int64 [.., 4]      x0, y0, x1, y1, inclusive
      "centroid" float64 [.., 2]  cx, cy = sum x / area, sum y / area (exact sums, one division each)
      "peak" float32      the maximum v
      "peak_index" int64  the smallest linear index that reaches it
      "gt_area" int64     pixels of the region with pixel_label != 0 (0 without pixel_label)"""
    if pixel_preds.dim() == 4 and pixel_preds.shape[1] == 1:
        pixel_preds = pixel_preds[:, 0]
    if pixel_preds.dim() != 3 or pixel_preds.numel() == 0:
        raise ValueError(f"pixel_preds must be a non-empty [n, H, W] or [n, 1, H, W], got {tuple(pixel_preds.shape)}")
    if int(min_area) < 1 or int(max_regions) < 1:
        raise ValueError(f"min_area and max_regions must be at least 1, got {min_area} and {max_regions}")
    preds = pixel_preds.to(torch.float32).contiguous()
    n, H, W = preds.shape
    lab = None
    if pixel_label is not None:
        if pixel_label.dim() == 4 and pixel_label.shape[1] == 1:
            pixel_label = pixel_label[:, 0]
        if tuple(pixel_label.shape) != (n, H, W):
            raise ValueError(f"pixel_label must match pixel_preds {(n, H, W)}, got {tuple(pixel_label.shape)}")
        lab = (pixel_label != 0).to(torch.uint8).contiguous()
    R = int(max_regions)
    with torch.cuda.device(preds.device):
        _dev(preds, lab)
        need = ctypes.c_size_t(0)
        call("aaclip_regions_workspace", n * H * W, n, ctypes.byref(need))
        ws, at = _aligned_workspace(int(need.value), preds.device)
        # the C side writes uint32; int32 storage holds the same bits
        i32 = {k: torch.empty(shape, device=preds.device, dtype=torch.int32)
               for k, shape in (("n_regions", (n,)), ("label", (n, R)), ("area", (n, R)), ("bbox", (n, R, 4)),
                                ("peak_index", (n, R)), ("gt_area", (n, R)))}
        centroid = torch.empty(n, R, 2, device=preds.device, dtype=torch.float64)
        peak = torch.empty(n, R, device=preds.device, dtype=torch.float32)
        call("aaclip_extract_regions", _ptr(preds), _ptr(lab), n, H, W, float(threshold), int(bool(normalise)),
             int(min_area), R, at, need.value, _ptr(i32["n_regions"]), _ptr(i32["label"]), _ptr(i32["area"]),
             _ptr(i32["bbox"]), _ptr(centroid), _ptr(peak), _ptr(i32["peak_index"]), _ptr(i32["gt_area"]), _stream())
        out = {k: v.to(torch.int64) & 0xFFFFFFFF for k, v in i32.items()}
        out["centroid"], out["peak"] = centroid, peak
        return out


_bilinear_plans: dict = {}


def bilinear_plan(in_size: int, out_size: int):
    """The per-axis table of aaclip_resize_bilinear_u8: int32 [out_size, 3] = (s, a0, a1). Host only."""
    import numpy as np
    table = np.zeros((int(out_size), 3), np.int32)
    call("aaclip_bilinear_plan", int(in_size), int(out_size), table.ctypes.data_as(ctypes.c_void_p))
    return table


def resize_bilinear_u8(src, size, out=None):
    """8-bit fixed-point bilinear resize on the device (aaclip_resize_bilinear_u8, the resize of
    forward_utils.visualize): src uint8 [B, h, w, 3] RGB (pixel rows contiguous; the row pitch and the
    image stride may be padded) -> uint8 [B, size, size, 3]. The per-axis tables are built on the
    host and cached per (source size, size, device)."""
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3 or src.numel() == 0:
        raise ValueError(f"src must be a non-empty uint8 [B, h, w, 3], got {src.dtype} {tuple(src.shape)}")
    if src.stride(3) != 1 or src.stride(2) != 3 or src.stride(1) < 3 * src.shape[2] or \
            (src.shape[0] > 1 and src.stride(0) < src.stride(1) * src.shape[1]):
        raise ValueError("pixel rows must be contiguous (the row pitch and the image stride may be padded)")
    S = int(size)
    if S < 1:
        raise ValueError(f"size must be at least 1, got {size}")
    if not src.is_cuda:
        raise RuntimeError("aaclip ops need device (HIP) tensors; there is no CPU path")
    B, h, w, _ = src.shape
    if out is None:
        out = torch.empty(B, S, S, 3, device=src.device, dtype=torch.uint8)
    if tuple(out.shape) != (B, S, S, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 {(B, S, S, 3)}")
    with torch.cuda.device(src.device):
        _dev(src, out)
        tables = []
        for n in (w, h):
            key = (n, S, src.device)
            if key not in _bilinear_plans:
                _bilinear_plans[key] = torch.from_numpy(bilinear_plan(n, S)).to(src.device)
            tables.append(_bilinear_plans[key])
        call("aaclip_resize_bilinear_u8", _ptr(src), src.stride(0), src.stride(1), B, h, w, _ptr(tables[0]),
             _ptr(tables[1]), S, _ptr(out), _stream())
    return out


def overlay_range(maps):
    """(lo, hi) of a class's maps as a device fp32 [2] (aaclip_overlay_range), without a host sync."""
    if maps.dim() < 2 or maps.numel() == 0:
        raise ValueError(f"maps must be a non-empty [n, ...], got {tuple(maps.shape)}")
    maps = maps.to(torch.float32).contiguous()
    n = maps.shape[0]
    with torch.cuda.device(maps.device):
        _dev(maps)
        need = ctypes.c_size_t(0)
        call("aaclip_overlay_workspace", n, ctypes.byref(need))
        ws = torch.empty(int(need.value) // 4, device=maps.device, dtype=torch.float32)
        out = torch.empty(2, device=maps.device, dtype=torch.float32)
        call("aaclip_overlay_range", _ptr(maps), n, maps.numel() // n, _ptr(ws), need.value, _ptr(out), _stream())
    return out


def overlay_panels(maps, thumbs, *, labels=None, value_range=None, swap_rb=True, out=None):
    """The three stacked panels of forward_utils.visualize (aaclip_overlay_panels): maps fp32
    [n, S, S] or [n, 1, S, S]; thumbs uint8 [n, S, S, 3] RGB; labels the maps' shape (nonzero =
    anomalous) or None; value_range a device fp32 [2] = (lo, hi) of the class (overlay_range) or
    None for no normalisation; swap_rb exchanges the photo's red and blue as the reference's files
    have them. Returns uint8 [n, 3 S, S, 3], enqueued without a host sync."""
    if maps.dim() == 4 and maps.shape[1] == 1:
        maps = maps[:, 0]
    if maps.dim() != 3 or maps.numel() == 0 or maps.shape[1] != maps.shape[2]:
        raise ValueError(f"maps must be a non-empty [n, S, S] or [n, 1, S, S], got {tuple(maps.shape)}")
    maps = maps.to(torch.float32).contiguous()
    n, S, _ = maps.shape
    if thumbs.dtype != torch.uint8 or tuple(thumbs.shape) != (n, S, S, 3):
        raise ValueError(f"thumbs must be uint8 {(n, S, S, 3)}, got {thumbs.dtype} {tuple(thumbs.shape)}")
    thumbs = thumbs.contiguous()
    lab = None
    if labels is not None:
        if labels.dim() == 4 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if tuple(labels.shape) != (n, S, S):
            raise ValueError(f"labels must match maps {(n, S, S)}, got {tuple(labels.shape)}")
        lab = (labels != 0).to(torch.uint8).contiguous()
    if value_range is not None:
        if value_range.dtype != torch.float32 or tuple(value_range.shape) != (2,):
            raise ValueError("value_range must be a device fp32 [2] = (lo, hi)")
        value_range = value_range.contiguous()
    if out is None:
        out = torch.empty(n, 3 * S, S, 3, device=maps.device, dtype=torch.uint8)
    if tuple(out.shape) != (n, 3 * S, S, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 {(n, 3 * S, S, 3)}")
    with torch.cuda.device(maps.device):
        _dev(maps, thumbs, lab, value_range, out)
        call("aaclip_overlay_panels", _ptr(maps), _ptr(lab), _ptr(thumbs), _ptr(value_range), n, S, int(bool(swap_rb)),
             _ptr(out), _stream())
    return out


def _metrics_eval_dev(preds, lab, ip, il, N, pix, medical):
    _dev(preds, lab, ip, il)
    need = ctypes.c_size_t(0)
    call("aaclip_metrics_workspace", N * pix, N, ctypes.byref(need))
    ws = torch.empty(int(need.value) + 256, device=preds.device, dtype=torch.uint8)
    off = (-ws.data_ptr()) % 256
    out = torch.empty(4, device=preds.device, dtype=torch.float64)
    call("aaclip_metrics_eval", _ptr(preds), _ptr(lab), _ptr(ip), _ptr(il), N, pix, int(medical),
         ws.data_ptr() + off, need.value, _ptr(out), _stream())
    return out


# ------------------------------------------------------------------------ few-shot memory bank
BANK_TM = 256          # AACLIP_BANK_TILE_M: query rows per block
BANK_TN = 256          # AACLIP_BANK_TILE_N: bank rows per tile
BANK_MAX_SPLITS = 64   # AACLIP_BANK_MAX_SPLITS
FUSE_HEAD = 256        # AACLIP_FEWSHOT_FUSE_HEAD


def bank_nn_plan(M: int, Nb: int):
    """(n_splits, tiles_per_split) of a bank_nn launch (aaclip_bank_nn_workspace; host only): split s
    owns the bank rows [s * tiles_per_split * BANK_TN, (s + 1) * tiles_per_split * BANK_TN)."""
    if int(M) < 1 or int(Nb) < 1:
        raise ValueError(f"bank_nn needs at least one query row and one bank row, got {M} and {Nb}")
    nbytes, n_splits = ctypes.c_size_t(0), ctypes.c_int(0)
    call("aaclip_bank_nn_workspace", int(M), int(Nb), ctypes.byref(nbytes), ctypes.byref(n_splits))
    tiles = -(-int(Nb) // BANK_TN)
    return n_splits.value, -(-tiles // n_splits.value)


def _bank_rows(t, name):
    _rowmajor(t, name)
    if t.shape[0] < 1:
        raise ValueError(f"bank_nn: {name} has no rows")
    if t.stride(0) < t.shape[1] or (t.stride(0) * t.element_size()) % 16 or t.data_ptr() % 16:
        raise ValueError(f"bank_nn: {name}'s rows must be 16-byte aligned, with a row stride of at least K")


def bank_nn(q, bank, part=None):
    """part[m, s] = max over the bank rows of split s of q[m] . bank[n] (aaclip_bank_nn): the
    nearest-patch search of the few-shot path, an MFMA GEMM that keeps only a running row maximum.
    q [M, K], bank [Nb, K]: float16, bfloat16 or float32, the same for both; unit column stride, any
    16-byte aligned row stride; K a multiple of 64; finite values. part: fp32 [M, n_splits] contiguous
    (bank_nn_plan) or None for a fresh one; returned. max over s is the row's result (bank_distance)."""
    _bank_rows(q, "q")
    _bank_rows(bank, "bank")
    if q.dtype != bank.dtype:
        raise TypeError(f"bank_nn operands must share a dtype, got {q.dtype} and {bank.dtype}")
    tag = dtag(q)
    M, K = q.shape
    Nb = bank.shape[0]
    if bank.shape[1] != K or K % 64 or K == 0:
        raise ValueError(f"bank_nn needs q [M, K] and bank [Nb, K] with K a multiple of 64, got {tuple(q.shape)} "
                         f"and {tuple(bank.shape)}")
    n_splits, _ = bank_nn_plan(M, Nb)
    if part is None:
        part = torch.empty(M, n_splits, device=q.device, dtype=torch.float32)
    if part.dtype != torch.float32 or tuple(part.shape) != (M, n_splits) or not part.is_contiguous():
        raise ValueError(f"bank_nn: part must be a contiguous float32 {(M, n_splits)} workspace, got {part.dtype} "
                         f"{tuple(part.shape)}")
    _dev(q, bank, part)  # after the shape / dtype checks: those need no device
    _launch("fewshot", "bank_nn", 2.0 * M * Nb * K, (M * K + Nb * K) * q.element_size() + 4.0 * part.numel(),
            "aaclip_bank_nn", tag, M, Nb, K, _ptr(q), q.stride(0), _ptr(bank), bank.stride(0), _ptr(part),
            part.numel() * 4, _stream())
    return part


class Fp8MxRows:
    """Unit rows in MX fp8, the operands of bank_nn_fp8mx (unit_rows_fp8mx): q uint8 [n, K], the e4m3
    bytes; sc uint8 [K / 128, ld, 2], the e8m0 block scales (mx_scales; ld even); rnorm fp32 [n], the
    reciprocal norm of each stored row. shape is q's, dtype torch.float8_e4m3fn."""
    dtype = torch.float8_e4m3fn

    def __init__(self, q, sc, rnorm):
        self.q, self.sc, self.rnorm = q, sc, rnorm

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    def __repr__(self):
        return f"Fp8MxRows(shape={tuple(self.q.shape)}, ld_sc={self.sc.shape[1]})"


def unit_rows_fp8mx(x):
    """The rows of x [n, K] (float32, bfloat16 or float16; unit column stride, 16-byte aligned rows; K a
    multiple of 128) L2-normalised as l2_normalize does it and MX-quantised to e4m3 by csrc/mxfp8.h's
    rule, with the reciprocal norm of every stored row (aaclip_unit_rows_fp8mx). Returns a fresh
    Fp8MxRows."""
    _rowmajor(x, "x")
    tag = dtag(x)
    n, K = x.shape
    if n < 1 or K == 0 or K % 128:
        raise ValueError(f"unit_rows_fp8mx needs x [n >= 1, K] with K a multiple of 128, got {tuple(x.shape)}")
    if x.stride(0) < K or (x.stride(0) * x.element_size()) % 16 or x.data_ptr() % 16:
        raise ValueError("unit_rows_fp8mx: x's rows must be 16-byte aligned, with a row stride of at least K")
    _dev(x)
    q = torch.empty(n, K, device=x.device, dtype=torch.uint8)
    sc = mx_scales(n, K, x.device)
    rnorm = torch.empty(n, device=x.device, dtype=torch.float32)
    _launch("fewshot", "unit_rows_fp8mx", 4.0 * n * K, n * K * (x.element_size() + 1.0) + 4.0 * n,
            "aaclip_unit_rows_fp8mx", tag, _ptr(x), x.stride(0), _ptr(q), q.stride(0), _ptr(sc), sc.shape[1],
            _ptr(rnorm), n, K, _stream())
    return Fp8MxRows(q, sc, rnorm)


def _mx_rows(t, name):
    if not isinstance(t, Fp8MxRows):
        raise TypeError(f"bank_nn_fp8mx: {name} must be an Fp8MxRows (unit_rows_fp8mx), got {type(t).__name__}")
    q, sc, rn = t.q, t.sc, t.rnorm
    _rowmajor(q, name)
    n, K = q.shape
    if n < 1:
        raise ValueError(f"bank_nn_fp8mx: {name} has no rows")
    if q.dtype not in (torch.uint8, torch.float8_e4m3fn):
        raise TypeError(f"bank_nn_fp8mx: {name}.q must hold e4m3 bytes (uint8 or float8_e4m3fn), got {q.dtype}")
    if q.stride(0) < K or q.stride(0) % 16 or q.data_ptr() % 16:
        raise ValueError(f"bank_nn_fp8mx: {name}'s rows must be 16-byte aligned, with a row stride of at least K")
    if (sc.dtype != torch.uint8 or sc.dim() != 3 or not sc.is_contiguous() or sc.shape[0] * 128 != K
            or sc.shape[1] < n or sc.shape[1] % 2 or sc.shape[2] != 2):
        raise ValueError(f"bank_nn_fp8mx: {name}.sc must be contiguous uint8 [K / 128, ld >= rows and even, 2], got "
                         f"{sc.dtype} {tuple(sc.shape)}")
    if rn.dtype != torch.float32 or tuple(rn.shape) != (n,) or not rn.is_contiguous():
        raise ValueError(f"bank_nn_fp8mx: {name}.rnorm must be contiguous float32 [{n}], got {rn.dtype} "
                         f"{tuple(rn.shape)}")


def bank_nn_fp8mx(q, bank, part=None):
    """bank_nn on MX fp8 operands (aaclip_bank_nn_fp8mx): part[m, s] = max over the bank rows of split s
    of the cosine between the stored rows, (q^[m] . bank^[n]) * bank.rnorm[n] * q.rnorm[m], on the
    block-scaled fp8 MFMA. q, bank: Fp8MxRows of one K, a multiple of 128 (any 16-byte aligned row
    stride). part as in bank_nn, with bank_nn_plan's layout; bank_distance takes it as it is."""
    _mx_rows(q, "q")
    _mx_rows(bank, "bank")
    M, K = q.shape
    Nb = bank.shape[0]
    if bank.shape[1] != K or K % 128 or K == 0:
        raise ValueError(f"bank_nn_fp8mx needs q [M, K] and bank [Nb, K] with K a multiple of 128, got "
                         f"{tuple(q.shape)} and {tuple(bank.shape)}")
    n_splits, _ = bank_nn_plan(M, Nb)
    if part is None:
        part = torch.empty(M, n_splits, device=q.device, dtype=torch.float32)
    if part.dtype != torch.float32 or tuple(part.shape) != (M, n_splits) or not part.is_contiguous():
        raise ValueError(f"bank_nn_fp8mx: part must be a contiguous float32 {(M, n_splits)} workspace, got "
                         f"{part.dtype} {tuple(part.shape)}")
    _dev(q.q, q.sc, q.rnorm, bank.q, bank.sc, bank.rnorm, part)
    _launch("fewshot", "bank_nn_fp8mx", 2.0 * M * Nb * K, (M + Nb) * (K + K / 64 + 4.0) + 4.0 * part.numel(),
            "aaclip_bank_nn_fp8mx", M, Nb, K, _ptr(q.q), q.q.stride(0), _ptr(q.sc), q.sc.shape[1], _ptr(q.rnorm),
            _ptr(bank.q), bank.q.stride(0), _ptr(bank.sc), bank.sc.shape[1], _ptr(bank.rnorm), _ptr(part),
            part.numel() * 4, _stream())
    return part


def bank_distance(part, grid, *, accumulate: bool):
    """grid[m] = (accumulate ? grid[m] : 0) + (1 - max_s part[m, s]) (aaclip_bank_distance). part fp32
    [M, n_splits] contiguous (bank_nn); grid contiguous fp32 of M elements, e.g. the [B, 1, g, g] grid
    blur_upsample takes (row m = b * g * g + p). Called per level, accumulate from the second on."""
    if part.dim() != 2 or part.dtype != torch.float32 or not part.is_contiguous() or part.numel() == 0:
        raise ValueError("bank_distance: part must be a non-empty contiguous float32 [M, n_splits]")
    M, n_splits = part.shape
    if n_splits > BANK_MAX_SPLITS:
        raise ValueError(f"bank_distance: at most {BANK_MAX_SPLITS} splits, got {n_splits}")
    if grid.dtype != torch.float32 or not grid.is_contiguous() or grid.numel() != M:
        raise ValueError(f"bank_distance: grid must be contiguous float32 of {M} elements, got {grid.dtype} "
                         f"{tuple(grid.shape)}")
    _dev(part, grid)
    _launch("fewshot", "bank_distance", 0.0, 4.0 * part.numel() + 8.0 * M, "aaclip_bank_distance", _ptr(part), M,
            n_splits, int(bool(accumulate)), _ptr(grid), _stream())
    return grid


CORESET_MAX_K = 4096        # AACLIP_CORESET_MAX_K
CORESET_BLOCK_ROWS = 64     # AACLIP_CORESET_BLOCK_ROWS: rows per slab
CORESET_MAX_BLOCKS = 512    # AACLIP_CORESET_MAX_BLOCKS: candidates per step


def coreset_rows(n: int, ratio: float) -> int:
    """Rows a coreset of `ratio` keeps of n: max(1, ceil(ratio * n)), for 0 < ratio <= 1."""
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError(f"a coreset ratio must lie in (0, 1], got {ratio}")
    if int(n) < 1:
        raise ValueError(f"a coreset needs at least one row, got {n}")
    return min(int(n), max(1, math.ceil(float(ratio) * int(n))))


def coreset_blocks(n: int) -> int:
    """Blocks (= candidates per step) of a bank_coreset launch on n rows: the slabs dealt evenly
    over the fewest grid-stride trips that stay within CORESET_MAX_BLOCKS (csrc/bank.hip)."""
    slabs = -(-int(n) // CORESET_BLOCK_ROWS)
    return -(-slabs // -(-slabs // CORESET_MAX_BLOCKS))


def bank_coreset(rows, m: int, start: int = 0):
    """Greedy k-centre coreset of rows [N, K] (aaclip_bank_coreset; tests/coreset_ref.py): from
    `start`, m - 1 times the row whose largest dot product with the rows picked so far is smallest,
    the lowest index on ties -- farthest-point selection under 1 - cosine when the rows are unit
    (normalising them is the caller's job). rows: float16, bfloat16 or float32, unit column stride,
    any 16-byte aligned row stride, K a multiple of 64 up to CORESET_MAX_K, finite values.
    Returns (sel int32 [m] in pick order, cover fp32 [m]: each pick's similarity to the picks
    before it (cover[0] = -inf), maxsim fp32 [N]: every row's largest similarity to a picked row).
    m launches on the current stream, no host sync."""
    _bank_rows(rows, "rows")
    tag = dtag(rows)
    N, K = rows.shape
    m, start = int(m), int(start)
    if K % 64 or K == 0 or K > CORESET_MAX_K:
        raise ValueError(f"bank_coreset needs rows [N, K] with K a multiple of 64 up to {CORESET_MAX_K}, got "
                         f"{tuple(rows.shape)}")
    if N > 1 << 30 or not 1 <= m <= N or not 0 <= start < N:
        raise ValueError(f"bank_coreset needs 1 <= m <= N <= 2^30 and 0 <= start < N, got m = {m}, start = {start}, "
                         f"N = {N}")
    _dev(rows)
    need = ctypes.c_size_t(0)
    call("aaclip_bank_coreset_workspace", N, ctypes.byref(need))
    ws, at = _aligned_workspace(int(need.value), rows.device)
    sel = torch.empty(m, device=rows.device, dtype=torch.int32)
    cover = torch.empty(m, device=rows.device, dtype=torch.float32)
    maxsim = torch.empty(N, device=rows.device, dtype=torch.float32)
    _launch("fewshot", "bank_coreset", 2.0 * m * N * K, float(m) * N * K * rows.element_size(),
            "aaclip_bank_coreset", tag, N, K, _ptr(rows), rows.stride(0), m, start, _ptr(sel), _ptr(cover),
            _ptr(maxsim), at, int(need.value), _stream())
    return sel, cover, maxsim


def fewshot_fuse(zs_map, fs_map, zs_score):
    """One class's zero-shot and few-shot results fused (aaclip_fewshot_fuse): zs_map / fs_map fp32
    [n, ...] of equal shapes, zs_score [n]. Returns (fused_map of zs_map's shape, fs_score [n],
    fused_score [n]): fs_score the per-image maximum of fs_map; fused = N(zero-shot) + N(few-shot),
    N the min-max normalisation over the class (0 for a constant input). Enqueued without a host
    sync; numpy float32 gives the same bits (tests/fewshot_ref.py)."""
    if zs_map.dim() < 2 or zs_map.numel() == 0 or tuple(fs_map.shape) != tuple(zs_map.shape):
        raise ValueError(f"fewshot_fuse: zs_map and fs_map must be non-empty [n, ...] of one shape, got "
                         f"{tuple(zs_map.shape)} and {tuple(fs_map.shape)}")
    n = zs_map.shape[0]
    if zs_score.numel() != n:
        raise ValueError(f"fewshot_fuse: zs_score must have one entry per image ({n}), got {tuple(zs_score.shape)}")
    for t, name in ((zs_map, "zs_map"), (fs_map, "fs_map"), (zs_score, "zs_score")):
        if t.dtype != torch.float32:
            raise TypeError(f"fewshot_fuse: {name} must be float32, got {t.dtype}")
    zs_map, fs_map, zs_score = zs_map.contiguous(), fs_map.contiguous(), zs_score.reshape(-1).contiguous()
    with torch.cuda.device(zs_map.device):
        _dev(zs_map, fs_map, zs_score)
        need = ctypes.c_size_t(0)
        call("aaclip_overlay_workspace", n, ctypes.byref(need))
        nbytes = FUSE_HEAD + int(need.value)
        ws, at = _aligned_workspace(nbytes, zs_map.device)
        fused_map = torch.empty_like(zs_map)
        fs_score = torch.empty(n, device=zs_map.device, dtype=torch.float32)
        fused_score = torch.empty(n, device=zs_map.device, dtype=torch.float32)
        call("aaclip_fewshot_fuse", _ptr(zs_map), _ptr(fs_map), _ptr(zs_score), n, zs_map.numel() // n, at, nbytes,
             _ptr(fused_map), _ptr(fs_score), _ptr(fused_score), _stream())
    return fused_map, fs_score, fused_score


# ------------------------------------------------------------------------ tiled inference
TILE_MAX_GRID = 8  # tiles per axis (csrc/tiles.hip)


def tile_canvas(S: int, G: int, O: int) -> int:
    """Canvas side of G x G tiles of side S overlapping by O pixels: G S - (G - 1) O. Raises
    ValueError outside 2 <= G <= 8, 0 <= O <= S // 2."""
    S, G, O = int(S), int(G), int(O)
    if S < 1 or not 2 <= G <= TILE_MAX_GRID or not 0 <= 2 * O <= S:
        raise ValueError(f"tiling needs a tile side >= 1, 2 <= grid <= {TILE_MAX_GRID} and 0 <= overlap <= side // 2, "
                         f"got side {S}, grid {G}, overlap {O}")
    return G * S - (G - 1) * O


def tile_side(C: int, G: int, O: int) -> int:
    """Tile side of a canvas of side C cut into G x G tiles overlapping by O: (C + (G - 1) O) / G,
    ValueError when that is no integer or the geometry is out of range."""
    C, G, O = int(C), int(G), int(O)
    if not 2 <= G <= TILE_MAX_GRID or O < 0 or C < 1 or (C + (G - 1) * O) % G:
        raise ValueError(f"a canvas of side {C} is not {G} x {G} tiles overlapping by {O} pixels")
    S = (C + (G - 1) * O) // G
    tile_canvas(S, G, O)
    return S


def tile_plan(S: int, G: int, O: int):
    """The per-axis tables of aaclip_tile_plan (host only): (index int32 [C, 2] = first covering
    tile, bilinear source cell i0; weight float32 [C, 4] = the first tile's weight, the next tile's
    or 0, 1 - lambda, lambda), C = tile_canvas(S, G, O). One pair serves rows and columns."""
    import numpy as np
    C = tile_canvas(S, G, O)
    index, weight = np.zeros((C, 2), np.int32), np.zeros((C, 4), np.float32)
    call("aaclip_tile_plan", int(S), int(G), int(O), index.ctypes.data_as(ctypes.c_void_p),
         weight.ctypes.data_as(ctypes.c_void_p))
    return index, weight


_tile_plans: dict = {}


def _tile_tables(S, G, O, device):
    key = (int(S), int(G), int(O), device)
    if key not in _tile_plans:
        index, weight = tile_plan(S, G, O)
        _tile_plans[key] = (torch.from_numpy(index).to(device), torch.from_numpy(weight).to(device))
    return _tile_plans[key]


def _tile_weight(global_weight, operand, name):
    a = float(global_weight)
    if not 0.0 <= a < 1.0:
        raise ValueError(f"{name}: global_weight must lie in [0, 1), got {global_weight}")
    if a > 0.0 and operand is None:
        raise ValueError(f"{name}: a global weight above 0 needs the global view's result")
    return a


def tile_gather(canvas, grid: int, overlap: int, *, images=None, tiles=None, out=None):
    """The tiles of a canvas as one batch (aaclip_tile_gather, a pure copy): canvas fp32 contiguous
    [n, 3, C, C] -> fp32 [k, 3, S, S], row b G^2 + ty G + tx = canvas[b, :, oy:oy+S, ox:ox+S] with
    the origin (ty, tx) (S - O). images = (b0, b1) gathers those images' tiles, tiles = (t0, t1)
    that run of tile rows (a chunk need not end on an image); neither = all of them."""
    if canvas.dim() != 4 or canvas.shape[1] != 3 or canvas.shape[2] != canvas.shape[3] or canvas.numel() == 0:
        raise ValueError(f"tile_gather: canvas must be a non-empty [n, 3, C, C], got {tuple(canvas.shape)}")
    if canvas.dtype != torch.float32 or not canvas.is_contiguous():
        raise ValueError("tile_gather: canvas must be contiguous float32")
    n, G, O = canvas.shape[0], int(grid), int(overlap)
    S = tile_side(canvas.shape[-1], G, O)
    if images is not None and tiles is not None:
        raise ValueError("tile_gather: give images or tiles, not both")
    t0, t1 = (0, n * G * G) if tiles is None else (int(tiles[0]), int(tiles[1]))
    if images is not None:
        t0, t1 = int(images[0]) * G * G, int(images[1]) * G * G
    if not 0 <= t0 < t1 <= n * G * G:
        raise ValueError(f"tile_gather: tile rows [{t0}, {t1}) lie outside the canvas batch's {n * G * G}")
    if out is None:
        out = torch.empty(t1 - t0, 3, S, S, device=canvas.device, dtype=torch.float32)
    if tuple(out.shape) != (t1 - t0, 3, S, S) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"tile_gather: out must be a contiguous float32 {(t1 - t0, 3, S, S)}")
    with torch.cuda.device(canvas.device):
        _dev(canvas, out)
        _launch("tiles", "tile_gather", 0.0, 8.0 * out.numel(), "aaclip_tile_gather", _ptr(canvas), n, S, G, O, t0,
                t1 - t0, _ptr(out), _stream())
    return out


def tile_stitch(tile_maps, grid: int, overlap: int, *, global_maps=None, global_weight: float = 0.0, out=None):
    """The tile maps put back together on the canvas (aaclip_tile_stitch): tile_maps fp32 contiguous
    [B G^2, S, S], image-major -> fp32 [B, C, C], every pixel the blend-weighted sum of the one, two
    or four tile pixels covering it; with global_weight a in (0, 1), (1 - a) times that plus a times
    global_maps [B, S, S] upsampled bilinearly (half-pixel centres). With a = 0 global_maps is not
    read. One writer per pixel in a fixed term order: deterministic. The tables are built on the
    host once per (S, G, O, device)."""
    G, O = int(grid), int(overlap)
    if tile_maps.dim() != 3 or tile_maps.shape[1] != tile_maps.shape[2] or tile_maps.numel() == 0 or \
            tile_maps.shape[0] % (G * G if 2 <= G <= TILE_MAX_GRID else 1):
        raise ValueError(f"tile_stitch: tile_maps must be a non-empty [B * {G * G}, S, S], got {tuple(tile_maps.shape)}")
    if tile_maps.dtype != torch.float32 or not tile_maps.is_contiguous():
        raise ValueError("tile_stitch: tile_maps must be contiguous float32")
    S = tile_maps.shape[-1]
    C = tile_canvas(S, G, O)
    B = tile_maps.shape[0] // (G * G)
    a = _tile_weight(global_weight, global_maps, "tile_stitch")
    if a == 0.0:
        global_maps = None
    elif tuple(global_maps.shape) != (B, S, S) or global_maps.dtype != torch.float32 or not global_maps.is_contiguous():
        raise ValueError(f"tile_stitch: global_maps must be a contiguous float32 {(B, S, S)}")
    if out is None:
        out = torch.empty(B, C, C, device=tile_maps.device, dtype=torch.float32)
    if tuple(out.shape) != (B, C, C) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"tile_stitch: out must be a contiguous float32 {(B, C, C)}")
    with torch.cuda.device(tile_maps.device):
        _dev(tile_maps, global_maps, out)
        index, weight = _tile_tables(S, G, O, tile_maps.device)
        nbytes = 4.0 * (out.numel() + tile_maps.numel() + (0 if global_maps is None else global_maps.numel()))
        _launch("tiles", "tile_stitch", 0.0, nbytes, "aaclip_tile_stitch", _ptr(tile_maps), _ptr(global_maps),
                _ptr(index), _ptr(weight), B, S, G, O, a, _ptr(out), _stream())
    return out


def tile_score(tile_scores, grid: int, *, global_scores=None, global_weight: float = 0.0, out=None):
    """Image scores of a tiled batch (aaclip_tile_score): tile_scores fp32 [B G^2] image-major ->
    fp32 [B] = (1 - a) max over the image's tiles + a global_scores[b]; with a = 0 the maximum
    itself. Enqueued without a host sync."""
    G = int(grid)
    if not 2 <= G <= TILE_MAX_GRID:
        raise ValueError(f"tile_score: 2 <= grid <= {TILE_MAX_GRID}, got {grid}")
    if tile_scores.dim() != 1 or tile_scores.numel() == 0 or tile_scores.numel() % (G * G):
        raise ValueError(f"tile_score: tile_scores must be a non-empty [B * {G * G}], got {tuple(tile_scores.shape)}")
    if tile_scores.dtype != torch.float32 or not tile_scores.is_contiguous():
        raise ValueError("tile_score: tile_scores must be contiguous float32")
    B = tile_scores.numel() // (G * G)
    a = _tile_weight(global_weight, global_scores, "tile_score")
    if a == 0.0:
        global_scores = None
    elif tuple(global_scores.shape) != (B,) or global_scores.dtype != torch.float32 or \
            not global_scores.is_contiguous():
        raise ValueError(f"tile_score: global_scores must be a contiguous float32 {(B,)}")
    if out is None:
        out = torch.empty(B, device=tile_scores.device, dtype=torch.float32)
    if tuple(out.shape) != (B,) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"tile_score: out must be a contiguous float32 {(B,)}")
    with torch.cuda.device(tile_scores.device):
        _dev(tile_scores, global_scores, out)
        _launch("tiles", "tile_score", 0.0, 4.0 * (tile_scores.numel() + 2 * B), "aaclip_tile_score",
                _ptr(tile_scores), _ptr(global_scores), B, G, a, _ptr(out), _stream())
    return out
