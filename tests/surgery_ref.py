"""Test support for the frozen CLIP image paths (not a test module).

  * vv_attention_ref: float64 numpy statement of aaclip_vv_attention: the reference's
    Attention (model/transformer.py:125-152) as the tower calls it, i.e. on [L, N, D]
    unpacked as [B, N, C], so the softmax runs across the images of the batch.
  * frozen_forward: torch-CPU restatement of VisionTransformer.forward
    (transformer.py:490-551), plain or after DAPM_replace, built on the oracle's
    prepare / _block plus the surgery block below. Pinned to the reference's goldens by
    tests/test_surgery_host.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import aaclip_torch as R
from oracle import synth

ROWS = [0, 1, 24, 25, 288, 300, 575, 576]
LEVELS = [6, 12, 18, 24]


def rel_l2(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def vv_attention_ref(v: np.ndarray, batch: int, n_tok: int, heads: int):
    """v [batch*n_tok, heads*64] -> (out float64 same shape, mean diagonal probability)."""
    x = np.asarray(v, dtype=np.float64).reshape(batch, n_tok, heads, 64)
    s = np.einsum("bthd,cthd->thbc", x, x) / 8.0
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    out = np.einsum("thbc,cthd->bthd", p, x).reshape(batch * n_tok, heads * 64)
    return out, float(np.einsum("thbb->thb", p).mean())


def vv_inputs(seed: int, batch: int, n_tok: int, heads: int) -> np.ndarray:
    """base[t] + 0.5 noise[b, t], unit normals: the images of a token position are close
    enough that the softmax really mixes them (plain randn gives a 0.998 diagonal)."""
    g = np.random.Generator(np.random.Philox(key=seed))
    base = g.standard_normal((1, n_tok, heads * 64), dtype=np.float32)
    noise = g.standard_normal((batch, n_tok, heads * 64), dtype=np.float32)
    return (base + 0.5 * noise).reshape(batch * n_tok, heads * 64).astype(np.float32)


def prepare(sd: dict, dtype=torch.float32) -> dict:
    """oracle prepare() of the tower (the adapters it also packs are not used here) + proj."""
    ia, _ = synth.adapter_state_dicts(111)
    w = R.prepare(sd, ia)
    w["proj"] = torch.as_tensor(np.asarray(sd["visual.proj"])).float()

    def cast(o):
        if isinstance(o, torch.Tensor):
            return o.to(dtype)
        if isinstance(o, dict):
            return {k: cast(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)) and not (o and isinstance(o[0], (int, bool))):
            return type(o)(cast(v) for v in o)
        return o
    return cast(w)


def surgery_block(x: torch.Tensor, b: dict, quick: bool = False) -> torch.Tensor:
    """A DAPM_replace'd block on token-major [B, N, D]: transformer.py:239-258 around the
    Attention of :125-152, whose returned x is proj(softmax_c(v_b . v_c / 8) v)."""
    B, N, D = x.shape
    H = R.HEADS
    h = F.layer_norm(x, (D,), b["ln1w"], b["ln1b"], 1e-5)
    v = F.linear(h, b["wqkv"][2 * D:], b["bqkv"][2 * D:]).view(B, N, H, D // H)
    p = torch.softmax(torch.einsum("bthd,cthd->thbc", v, v) * (D // H) ** -0.5, dim=-1)
    o = torch.einsum("thbc,cthd->bthd", p, v).reshape(B, N, D)
    x = x + F.linear(o, b["wo"], b["bo"])
    h = F.layer_norm(x, (D,), b["ln2w"], b["ln2b"], 1e-5)
    return x + F.linear(R._act(F.linear(h, b["wfc"], b["bfc"]), quick), b["wpr"], b["bpr"])


@torch.no_grad()
def frozen_forward(w: dict, x, out_layers, surgery_from=None):
    """(pooled [B, 768], [tokens [B, n_tok, 1024] after block i for i in out_layers])."""
    dt = w["cls"].dtype
    x = torch.as_tensor(x).to(dt)
    B, C, S, _ = x.shape
    g = S // R.PATCH
    cols = x.reshape(B, C, g, R.PATCH, g, R.PATCH).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, -1)
    x = cols @ w["conv"].T
    x = torch.cat([w["cls"].expand(B, 1, -1), x], 1) + w["pos"]
    x = F.layer_norm(x, (R.WIDTH,), *w["ln_pre"], 1e-5)
    tokens = []
    for i, b in enumerate(w["blocks"]):
        if surgery_from is not None and i >= surgery_from:
            x = surgery_block(x, b, w["quick"])
        else:
            x = R._block(x, b, w["quick"])
        if i + 1 in out_layers:
            tokens.append(x)
    pooled = F.layer_norm(x[:, 0], (R.WIDTH,), *w["ln_post"], 1e-5) @ w["proj"]
    return pooled, tokens


def patch_project(w: dict, tokens: torch.Tensor) -> torch.Tensor:
    """ln_post(tokens[:, 1:]) @ proj (model/adapter.py:58-62, train.py:78-81)."""
    return F.layer_norm(tokens[:, 1:], (R.WIDTH,), *w["ln_post"], 1e-5) @ w["proj"]
