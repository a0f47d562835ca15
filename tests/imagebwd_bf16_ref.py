"""The bf16 mixed-precision stage-2 step (VisualEngine.forward_train on a bf16 engine) restated in
fp32 torch on the CPU, on top of tests/imagebwd_ref.py: the same formulas, rounded to bf16 where
the recipe stores bf16. It is the YARDSTICK of tests/test_imagebwd_bf16_gpu.py: the device's error
against fp64 (imagebwd_ref.run / imagebwd_ref.block / fp64 autograd) may be at most 2 x this
restatement's error against the same fp64.

rnd(t, fwd, bwd) is one autograd Function: it rounds t to bf16 and back in its forward (fwd) and
the incoming gradient the same way in its backward (bwd).

Rounding points, forward (each stored in bf16 by the engine):
  * every GEMM weight: conv1, in_proj (the Q rows after log2(e)/8 is folded in, as the engine
    packs them), out_proj, c_fc, c_proj, and the 11 adapter weights at each call;
  * the im2col columns; h = ln_1(x) and ln_2(x); qkv; the attention output (inside: P before
    P.V and the row sum, as aaclip_attention does); fc = GELU(fc_pre) (fc_pre itself stays fp32);
    xb, the copy of x the adapter GEMM reads; the level taps ln_post(x[:, 1:]).
  The residual stream x, u, the blend, the projection outputs and everything after stay fp32.
Rounding points, backward:
  * the copy of g that feeds steps 1 and 5 of a block (g itself stays fp32);
  * d_act (step 1's output), d_pre (after GELU'), d_att (step 5's output), d_qkv;
  * inside the attention backward: P before P^T.dO, dS = P (dP - D) before dS.K and dS^T.Q
    (formed from the fp32 P), the three outputs;
  * the copy of du that feeds the adapter's input-gradient GEMM, the copy of the projection
    gradients that feeds dtap.
  The gradients of h (steps 3 and 7 write fp32), of the taps, of x and u, every LayerNorm
  backward and every weight gradient (fp32 dy^T x, x = the fp32 pre-blend stream for a layer
  adapter and the exactly upcast bf16 tap for a projection) stay fp32.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import imagebwd_ref as IR

LOG2E = 1.4426950408889634
Q_SCALE = 0.125 * LOG2E  # the engine's Q_LOG2_SCALE
LN2 = math.log(2.0)
BF16_EPS = 2.0 ** -8     # one bf16 ulp of a value in [1, 2)
GEMM_WEIGHTS = ("conv1.weight", "attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


def r(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even) and back, no autograd."""
    return t.to(torch.bfloat16).to(t.dtype)


class _Rnd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, fwd, bwd):
        ctx.bwd = bwd
        return r(t) if fwd else t.clone()

    @staticmethod
    def backward(ctx, g):
        return (r(g) if ctx.bwd else g), None, None


def rnd(t, fwd=True, bwd=True):
    return _Rnd.apply(t, fwd, bwd)


def _heads(t, B, N, H):
    return t.reshape(B, N, H, 64).transpose(1, 2)


def _merge(t, B, N, H):
    return t.transpose(1, 2).reshape(B * N, H * 64)


class _Attn16(torch.autograd.Function):
    """aaclip_attention (bf16) forward and aaclip_attention_bwd16 backward on packed qkv [B*N, 3*H*64]
    that holds bf16 values, rounding where the kernels round."""

    @staticmethod
    def forward(ctx, qkv, B, N, H, prescaled):
        q, k, v = (_heads(t, B, N, H) for t in qkv.split(H * 64, dim=-1))
        qp = q if prescaled else r(q * Q_SCALE)
        s = qp @ k.transpose(-1, -2)                      # log2 domain
        m = s.max(-1, keepdim=True).values
        p = torch.exp2(s - m)
        pb = r(p)
        out = r((pb @ v) / pb.sum(-1, keepdim=True))
        lse = m + torch.log2(p.sum(-1, keepdim=True))     # the backward's own pass 1, fp32 P
        ctx.save_for_backward(qp, k, v, out, s, lse)
        ctx.dims = (B, N, H, prescaled)
        return _merge(out, B, N, H)

    @staticmethod
    def backward(ctx, dout):
        qp, k, v, out, s, lse = ctx.saved_tensors
        B, N, H, prescaled = ctx.dims
        do = _heads(r(dout), B, N, H)
        P = torch.exp2(s - lse)
        dP = do @ v.transpose(-1, -2)
        D = (do * out).sum(-1, keepdim=True)
        dS = r(P * (dP - D))
        dv = r(P).transpose(-1, -2) @ do
        dq = (dS @ k) * (LN2 if prescaled else 0.125)
        dk = (dS.transpose(-1, -2) @ qp) * LN2
        return r(torch.cat([_merge(t, B, N, H) for t in (dq, dk, dv)], dim=-1)), None, None, None, None


def attention16(qkv, B, N, H, prescaled):
    return _Attn16.apply(qkv, B, N, H, prescaled)


def attention_truth(qkv, B, N, H, prescaled):
    """The same function without a rounding, differentiable by autograd in qkv's dtype (fp64: truth)."""
    q, k, v = (_heads(t, B, N, H) for t in qkv.split(H * 64, dim=-1))
    s = (q @ k.transpose(-1, -2)) * (LN2 if prescaled else 0.125)
    return _merge(torch.softmax(s, dim=-1) @ v, B, N, H)


class _Lin16(torch.autograd.Function):
    """y = rnd(x) rnd(w)^T of a trainable fp32 w: dx = rnd(dy) rnd(w) (the bf16 input-gradient GEMM
    on the bf16 copy of dy), dw = dy^T x in fp32 (aaclip_linear_wgrad on the fp32 x)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return r(x) @ r(w).T

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        lead = dy.reshape(-1, dy.shape[-1])
        return r(dy) @ r(w), lead.T @ x.reshape(-1, x.shape[-1])


def params16(sd: dict, prescale: bool = True, dtype=torch.float32) -> dict:
    """The visual tower as a bf16 engine packs it, held in `dtype`: GEMM weights rounded to bf16 (the Q
    rows of in_proj, weight and bias, times log2(e)/8 first when prescale), the rest fp32."""
    P = {}
    for k, v in sd.items():
        if not k.startswith("visual."):
            continue
        t = torch.as_tensor(np.asarray(v)).float().clone()
        if prescale and k.endswith(("attn.in_proj_weight", "attn.in_proj_bias")):
            t[:IR.WIDTH] *= Q_SCALE
        if k.endswith(GEMM_WEIGHTS):
            t = r(t)
        P[k] = t.to(dtype)
    return P


def unscaled(P16: dict, dtype=torch.float64) -> dict:
    """params16(prescale=True) with the Q rows divided by log2(e)/8 again, in `dtype`: the weights the
    packed tower stands for, in the layout imagebwd_ref.block takes."""
    P = {}
    for k, v in P16.items():
        t = v.to(dtype).clone()
        if k.endswith(("attn.in_proj_weight", "attn.in_proj_bias")):
            t[:IR.WIDTH] /= Q_SCALE
        P[k] = t
    return P


def _act(x, quick):
    return x * torch.sigmoid(1.702 * x) if quick else F.gelu(x)


def block16(P, i, x, quick=False, prescaled=True):
    """One frozen block of the bf16 step on the fp32 stream x [B, N, W]; P = params16(prescale=prescaled)."""
    p = f"visual.transformer.resblocks.{i}."
    B, N, W = x.shape
    H = W // 64
    ln = lambda t, n: F.layer_norm(t, (W,), P[p + n + ".weight"], P[p + n + ".bias"], 1e-5)  # noqa: E731
    h = rnd(ln(x, "ln_1"), bwd=False)
    qkv = rnd(h @ P[p + "attn.in_proj_weight"].T + P[p + "attn.in_proj_bias"])
    att = attention16(qkv.reshape(B * N, 3 * W), B, N, H, prescaled).reshape(B, N, W)
    x = x + rnd(att @ P[p + "attn.out_proj.weight"].T + P[p + "attn.out_proj.bias"], fwd=False)
    h = rnd(ln(x, "ln_2"), bwd=False)
    fc_pre = rnd(h @ P[p + "mlp.c_fc.weight"].T + P[p + "mlp.c_fc.bias"], fwd=False)
    fc = rnd(_act(fc_pre, quick))
    return x + rnd(fc @ P[p + "mlp.c_proj.weight"].T + P[p + "mlp.c_proj.bias"], fwd=False)


def forward16(P, ws, x, *, levels=IR.LEVELS, adapt_until=6, i_w=0.1, relu=False, quick=False, taps=None):
    """imagebwd_ref.forward in the bf16 recipe. P = params16(sd); ws: the fp32 adapter weights."""
    B, C, S, _ = x.shape
    g = S // IR.PATCH
    cols = x.reshape(B, C, g, IR.PATCH, g, IR.PATCH).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, C * IR.PATCH * IR.PATCH)
    t = r(cols) @ P["visual.conv1.weight"].reshape(IR.WIDTH, -1).T
    t = torch.cat([P["visual.class_embedding"].expand(B, 1, -1), t], 1) + P["visual.positional_embedding"]
    t = F.layer_norm(t, (IR.WIDTH,), P["visual.ln_pre.weight"], P["visual.ln_pre.bias"], 1e-5)
    tokens = []
    for i in range(max(levels)):
        t = block16(P, i, t, quick)
        if taps is not None and i in taps:
            if t.requires_grad:
                t.retain_grad()
            else:
                t.requires_grad_()
            taps[i] = t
        if i < adapt_until:
            u = F.leaky_relu(_Lin16.apply(t, ws[i]), 0.01)
            u = u * t.norm(dim=-1, keepdim=True) / u.norm(dim=-1, keepdim=True)
            t = i_w * u + (1 - i_w) * t
        if i + 1 in levels:
            tokens.append(t[:, 1:])
    tokens = [rnd(F.layer_norm(v, (IR.WIDTH,), P["visual.ln_post.weight"], P["visual.ln_post.bias"], 1e-5), bwd=False)
              for v in tokens]
    proj = lambda v, w: F.leaky_relu(_Lin16.apply(v, w), 0.01) if relu else _Lin16.apply(v, w)  # noqa: E731
    L = len(levels)
    seg = [F.normalize(proj(v, ws[adapt_until + j]), dim=-1) for j, v in enumerate(tokens)]
    det = F.normalize(proj(tokens[-1], ws[adapt_until + L]), dim=-1).mean(1)
    return seg, det


def run16(sd, adapter, x, G, *, adapt_until=6, levels=IR.LEVELS, relu=False, quick=False, P=None, trainable=None):
    """imagebwd_ref.run for the bf16 recipe, in fp32 on the CPU: seg, det, loss, grads and taps as numpy."""
    P = params16(sd) if P is None else P
    names = IR.weight_names(adapt_until, len(levels), relu)
    ws = [torch.as_tensor(np.asarray(adapter[n])).float() for n in names]
    for i, w in enumerate(ws):
        if trainable is None or i in trainable:
            w.requires_grad_()
    taps = {i: None for i in IR.TAPS if i < max(levels)}
    seg, det = forward16(P, ws, torch.as_tensor(np.asarray(x)).float(), levels=levels, adapt_until=adapt_until,
                         relu=relu, quick=quick, taps=taps)
    loss = IR.fixture_loss(seg, det, [torch.as_tensor(g).float() for g in G])
    loss.backward()
    tap_g = {i: (t.grad[0].numpy() if t.grad is not None else np.zeros(tuple(t.shape[1:]))) for i, t in taps.items()}
    return dict(seg=[s.detach().numpy() for s in seg], det=det.detach().numpy(), loss=float(loss.detach()),
                grads=[w.grad.numpy() if w.grad is not None else None for w in ws], taps=tap_g)


def worst_row(a, b) -> float:
    """The largest rel-L2 of a row of a against the same row of b ([rows, cols] each)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, np.shape(a)[-1])
    b = np.asarray(b, dtype=np.float64).reshape(a.shape)
    return float((np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)).max())
