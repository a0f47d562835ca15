"""Independent torch restatement of the stage-1 loss head (reference train.py:86-100,
forward_utils.py:21-126, :196-227), written from the formulas, differentiable by autograd.
It runs in whatever dtype its inputs have: fp64 is the truth the GPU tests compare with,
fp32 on the CPU is the yardstick (the error the reference's own arithmetic has).
tests/test_segloss_host.py pins it to the real reference's golden_segloss.npz.

  logits(f, T)              [B, L, 768] x ([768, 2] | [B, 768, 2]) -> grid [B, 2, g, g]
  upsample_softmax(grid, S) bilinear align_corners -> softmax over the 2 channels
  seg_loss(probs, mask)     (total, focal, dice0, dice1, sums [B, 7])
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

SHAPES = [(1, 2, 3), (3, 5, 23), (2, 24, 336), (2, 37, 518)]  # (B, g, S)
SMOOTH = 1e-5


def rel_l2(a, b) -> float:
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def unit_rows(rng, *shape):
    x = rng.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def inputs(seed, B, g, S, per_image=True):
    """Unit-norm random features [B, g*g, 768] and anchors ([B, 768, 2] or [768, 2]) as fp32
    numpy, and a mask [B, 1, S, S]: image 0 a partial blob, image 1 all zero, image 2 all one
    (then repeating), the dice edge terms."""
    rng = np.random.default_rng(seed)
    f = unit_rows(rng, B, g * g, 768).astype(np.float32)
    Tn = unit_rows(rng, *((B, 2, 768) if per_image else (2, 768)))
    T = np.ascontiguousarray(np.swapaxes(Tn, -1, -2)).astype(np.float32)
    mask = np.zeros((B, 1, S, S), np.float32)
    yy, xx = np.mgrid[0:S, 0:S]
    for b in range(B):
        if b % 3 == 0:
            cy, cx, r = (0.3 + 0.1 * b) * S, 0.6 * S, 0.3 * S
            mask[b, 0] = (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r) | ((yy == S - 1) & (xx == S - 1))
        elif b % 3 == 2:
            mask[b, 0] = 1.0
    return f, T, mask


def logits(f, T):
    """100 * f @ T, channel-major on the square grid: [B, 2, g, g]."""
    B, L, _ = f.shape
    g = int(round(L ** 0.5))
    z = 100.0 * torch.matmul(f, T)  # T [768, 2] broadcasts, [B, 768, 2] is per image
    return z.permute(0, 2, 1).reshape(B, 2, g, g)


def upsample_softmax(grid, S):
    return torch.softmax(F.interpolate(grid, size=S, mode="bilinear", align_corners=True), dim=1)


def seg_loss(probs, mask):
    """probs [B, 2, S, S], mask [B, S, S] (same dtype). Returns (total, focal, dice0, dice1, sums)
    with sums [B, 7] = sum term, sum p0 t0, sum p0, sum t0, sum p1 t1, sum p1, sum t1."""
    B = probs.shape[0]
    p0, p1 = probs[:, 0].reshape(B, -1), probs[:, 1].reshape(B, -1)
    m = mask.reshape(B, -1)
    k = m.to(torch.int64)
    # the reference builds its one-hot in fp32 whatever the logits' dtype, so the clamp bounds
    # are the fp32 roundings of 1 - 1e-5 and 1e-5 in every precision (forward_utils.py:89-97)
    hi = torch.tensor(float(np.float32(1.0 - SMOOTH)), dtype=probs.dtype)
    lo = torch.tensor(float(np.float32(SMOOTH)), dtype=probs.dtype)
    o0, o1 = torch.where(k == 0, hi, lo), torch.where(k == 1, hi, lo)
    pt = (o0 * p0 + o1 * p1) + SMOOTH
    term = -((1 - pt) ** 2) * torch.log(pt)
    t0, t1 = 1 - m, m
    sums = torch.stack([term.sum(1), (p0 * t0).sum(1), p0.sum(1), t0.sum(1), (p1 * t1).sum(1), p1.sum(1),
                        t1.sum(1)], dim=1)
    focal = sums[:, 0].sum() / (B * m.shape[1])
    dice0 = 1 - ((2 * sums[:, 1] + 1) / (sums[:, 2] + sums[:, 3] + 1)).sum() / B
    dice1 = 1 - ((2 * sums[:, 4] + 1) / (sums[:, 5] + sums[:, 6] + 1)).sum() / B
    return (focal + dice0) + dice1, focal, dice0, dice1, sums


def run(f, T, mask, S, dtype=torch.float64, dloss=1.0):
    """The whole head in `dtype` on the CPU with autograd: dict of numpy arrays (loss terms,
    sums, grid, probs and the gradients dprobs, dgrid, dT, df)."""
    f = torch.as_tensor(f).to(dtype).requires_grad_()
    T = torch.as_tensor(T).to(dtype).requires_grad_()
    m = torch.as_tensor(mask).to(dtype).reshape(f.shape[0], S, S)
    grid = logits(f, T)
    grid.retain_grad()
    probs = upsample_softmax(grid, S)
    probs.retain_grad()
    total, focal, dice0, dice1, sums = seg_loss(probs, m)
    (total * dloss).backward()
    n = lambda t: t.detach().numpy()  # noqa: E731
    return dict(loss=n(total), focal=n(focal), dice0=n(dice0), dice1=n(dice1), sums=n(sums), grid=n(grid),
                probs=n(probs), dprobs=n(probs.grad), dgrid=n(grid.grad), dT=n(T.grad), df=n(f.grad))
