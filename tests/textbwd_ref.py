"""Independent torch restatement of the adapted text path (reference model/adapter.py:114-145,
forward_utils.py:138-162), written from the formulas and differentiable by autograd on the CPU.
It runs in whatever dtype it is asked for: fp64 is the truth the GPU tests compare with, fp32 on
the CPU is the yardstick (the error the reference's own arithmetic has).
tests/test_textbwd_host.py pins it to the real reference's golden_textbwd.npz.

  encode(P, ws, tokens)       [n, 77] ids -> [n, 768] (12 pre-LN causal blocks, the adapters after
                              blocks i < adapt_until, ln_final at the EOT row, LeakyReLU(eot W_out^T))
  anchor(emb)                 normalize(mean_s normalize(emb_s))
  run(sd, ad, tn, ta, G, dt)  loss L = sum G * T + 0.1 (T[:, 0] . T[:, 1])^2 on one class, backward:
                              T, the four weight gradients, dL/dx after the tapped blocks
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

TAPS = (11, 6, 2, 0)   # blocks whose output gradient the fixture stores (sentence 0 of the normal state)
ROWS = list(range(5, 768, 48))  # the 16 rows of each [768, 768] weight gradient the fixture stores in fp64
G_SEED = 901
ADAM_SEED = 902
ADAM_CLASSES = ["bottle", "bottle", "cable"]


def rel_l2(a, b) -> float:
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def loss_weights(seed=G_SEED):
    """The seeded G [768, 2] of the fixture's loss."""
    return np.random.default_rng(seed).standard_normal((768, 2)).astype(np.float32)


def params(sd: dict, dtype) -> dict:
    """The text tower's tensors out of a CLIP state dict (numpy or torch), in dtype."""
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()
            if not k.startswith("visual.") and k != "logit_scale"}


def _act(x, quick):
    return x * torch.sigmoid(1.702 * x) if quick else F.gelu(x)


def block(P, i, x, quick=False):
    """One pre-LN causal residual block on x [n, L, W]."""
    p = f"transformer.resblocks.{i}."
    n, L, W = x.shape
    H = W // 64
    h = F.layer_norm(x, (W,), P[p + "ln_1.weight"], P[p + "ln_1.bias"], 1e-5)
    qkv = h @ P[p + "attn.in_proj_weight"].T + P[p + "attn.in_proj_bias"]
    q, k, v = (t.reshape(n, L, H, 64).transpose(1, 2) for t in qkv.split(W, dim=-1))
    s = (q @ k.transpose(-1, -2)) / 8.0
    mask = torch.full((L, L), float("-inf"), dtype=x.dtype, device=x.device).triu_(1)
    a = torch.softmax(s + mask, dim=-1) @ v
    a = a.transpose(1, 2).reshape(n, L, W)
    x = x + a @ P[p + "attn.out_proj.weight"].T + P[p + "attn.out_proj.bias"]
    h = F.layer_norm(x, (W,), P[p + "ln_2.weight"], P[p + "ln_2.bias"], 1e-5)
    f = _act(h @ P[p + "mlp.c_fc.weight"].T + P[p + "mlp.c_fc.bias"], quick)
    return x + f @ P[p + "mlp.c_proj.weight"].T + P[p + "mlp.c_proj.bias"]


def encode(P, ws, tokens, *, adapt_until=3, t_w=0.1, quick=False, taps=None):
    """tokens [n, ctx] int64 -> [n, embed]. ws: adapt_until adapter weights + the output weight.
    taps: a dict {block: None} filled with the block outputs (pre-blend, grads retained)."""
    tokens = (tokens if isinstance(tokens, torch.Tensor) else torch.as_tensor(np.asarray(tokens))).long()
    tokens = tokens.to(P["positional_embedding"].device)
    eot = tokens.argmax(-1)
    L = int(eot.max()) + 1  # the tower is causal: nothing after the last EOT reaches an EOT row
    x = P["token_embedding.weight"][tokens[:, :L]] + P["positional_embedding"][:L]
    nb = len({k.split(".")[2] for k in P if k.startswith("transformer.resblocks.")})
    for i in range(nb):
        x = block(P, i, x, quick)
        if taps is not None and i in taps:
            if x.requires_grad:
                x.retain_grad()
            else:  # nothing trainable below (block 0): make the output a leaf so it collects a gradient
                x.requires_grad_()
            taps[i] = x
        if i < adapt_until:
            u = F.leaky_relu(x @ ws[i].T, 0.01)
            u = u * x.norm(dim=-1, keepdim=True) / u.norm(dim=-1, keepdim=True)
            x = t_w * u + (1 - t_w) * x
    x = F.layer_norm(x, (x.shape[-1],), P["ln_final.weight"], P["ln_final.bias"], 1e-5)
    return F.leaky_relu(x[torch.arange(x.shape[0], device=x.device), eot] @ ws[-1].T, 0.01)


def anchor(emb):
    e = emb / emb.norm(dim=-1, keepdim=True)
    m = e.mean(dim=0)
    return m / m.norm()


def class_anchors(P, ws, tok_normal, tok_abnormal, **kw):
    taps = kw.pop("taps", None)
    cols = [anchor(encode(P, ws, tok_normal, taps=taps, **kw)), anchor(encode(P, ws, tok_abnormal, **kw))]
    return torch.stack(cols, dim=1)


def fixture_loss(T, G):
    return (G * T).sum() + 0.1 * (T[:, 0] * T[:, 1]).sum() ** 2


def run(sd, adapter, tok_normal, tok_abnormal, G, dtype=torch.float64, *, adapt_until=3, quick=False, P=None):
    """One class's anchors, the fixture loss and its backward in `dtype` on the CPU. Returns
    numpy: T, loss, grads (list of the adapt_until + 1 weight gradients) and taps {block: dL/dx of
    the normal state's sentence 0, tokens 0..EOT}."""
    P = params(sd, dtype) if P is None else P
    ws = [torch.as_tensor(np.asarray(adapter[f"{i}.fc.0.weight"])).to(dtype).requires_grad_()
          for i in range(adapt_until + 1)]
    taps = {i: None for i in TAPS}
    T = class_anchors(P, ws, tok_normal, tok_abnormal, adapt_until=adapt_until, quick=quick, taps=taps)
    loss = fixture_loss(T, torch.as_tensor(G).to(dtype))
    loss.backward()
    n_eot = int(np.asarray(tok_normal)[0].argmax()) + 1
    tap_g = {i: (t.grad[0, :n_eot].numpy() if t.grad is not None else np.zeros((n_eot, t.shape[-1])))
             for i, t in taps.items()}
    return dict(T=T.detach().numpy(), loss=float(loss.detach()),
                grads=[w.grad.numpy() if w.grad is not None else None for w in ws], taps=tap_g)
