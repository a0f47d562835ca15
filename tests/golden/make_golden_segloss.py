"""Generate tests/golden/golden_segloss.npz by running the REAL reference's stage-1 loss
head (build machine only; needs the reference checkout make_golden.py names).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segloss.py

The reference's own calculate_similarity_map + calculate_seg_loss + loss.backward()
(train.py:86-100, forward_utils.py:21-126, :196-227) on the CPU, in fp32 and in fp64, on
tests/segloss_ref.inputs (unit-norm random f and T):

  case a  B=3, g=5,  S=23   per-image anchors [3, 768, 2]; masks: a partial blob, all zero, all one
  case b  B=2, g=24, S=336  shared anchors [768, 2]; masks: a partial blob, all zero

Stored per case: the inputs (case b's f is too large to commit: its seed, the rows ROWS_B and
a checksum are stored, segloss_ref.inputs regenerates it), loss{32,64} and the three
components, the 7 per-image sums (fp64), dT{32,64}, dgrid64, df64 at the rows ROWS_A / ROWS_B
(df is 100 * dgrid . T^T: the rows lose nothing) and dprobs64 (case b: every PIX_STEP-th
pixel). Also the share of pixels with p in (0.05, 0.95), and three Adam steps (betas (0.5, 0.999) as train.py:263-267, lr 1e-3) on
case a's anchors in fp32: the four losses, asserted here to fall at every step.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from make_golden import HERE, REPO  # noqa: E402 (sets sys.path: stubs, the reference, the repository)

sys.path.insert(0, os.path.join(REPO, "tests"))
import forward_utils as fu  # noqa: E402 (the reference's)
import segloss_ref as SR  # noqa: E402

SEED_A, SEED_B = 811, 812
ROWS_A = list(range(0, 75, 3))  # rows of case a's [B * g * g, 768] features whose df64 is stored
ROWS_B = [0, 1, 23, 24, 300, 575, 576, 1151]  # rows of case b's [B * g * g, 768] features
PIX_STEP = 97


def reference_run(f, T, mask, S, dtype):
    """train.py:89-90 + :99 as written there."""
    f = torch.from_numpy(f).to(dtype).requires_grad_()
    epoch_text_feature = torch.from_numpy(T).to(dtype).requires_grad_()
    mask = torch.from_numpy(mask).to(dtype)
    grabbed = {}
    interpolate = fu.F.interpolate

    def spy(x, *a, **k):  # the logits grid and the probabilities, for their gradients
        x.retain_grad()
        grabbed["grid"] = x
        return interpolate(x, *a, **k)

    fu.F.interpolate = spy
    try:
        patch_preds = fu.calculate_similarity_map(f, epoch_text_feature, S)
    finally:
        fu.F.interpolate = interpolate
    patch_preds.retain_grad()
    loss = fu.calculate_seg_loss(patch_preds, mask)
    focal = fu.focal_loss(patch_preds, mask)
    dice0 = fu.dice_loss(patch_preds[:, 0, :, :], 1 - mask)
    dice1 = fu.dice_loss(patch_preds[:, 1, :, :], mask)
    loss.backward()
    n = lambda t: t.detach().numpy()  # noqa: E731
    return dict(loss=n(loss), focal=n(focal), dice0=n(dice0), dice1=n(dice1), probs=n(patch_preds),
                dprobs=n(patch_preds.grad), dgrid=n(grabbed["grid"].grad), dT=n(epoch_text_feature.grad), df=n(f.grad))


def sums64(probs, mask):
    """The 7 per-image sums from the reference's own fp64 probabilities."""
    B = probs.shape[0]
    p0, p1 = probs[:, 0].reshape(B, -1), probs[:, 1].reshape(B, -1)
    m = mask.astype(np.float64).reshape(B, -1)
    o = np.float64(np.float32(1.0 - 1e-5)), np.float64(np.float32(1e-5))
    k = m.astype(np.int64)
    pt = np.where(k == 0, o[0], o[1]) * p0 + np.where(k == 1, o[0], o[1]) * p1 + 1e-5
    term = -((1 - pt) ** 2) * np.log(pt)
    return np.stack([term.sum(1), (p0 * (1 - m)).sum(1), p0.sum(1), (1 - m).sum(1), (p1 * m).sum(1), p1.sum(1),
                     m.sum(1)], axis=1)


def adam_losses(f, T, mask, S):
    f, mask = torch.from_numpy(f), torch.from_numpy(mask)
    T = torch.from_numpy(T.copy()).requires_grad_()
    opt = torch.optim.Adam([T], lr=1e-3, betas=(0.5, 0.999))
    losses = []
    for _ in range(3):
        loss = fu.calculate_seg_loss(fu.calculate_similarity_map(f, T, S), mask)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(fu.calculate_seg_loss(fu.calculate_similarity_map(f, T, S), mask)))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses  # the reference's loss falls at each step
    return np.array(losses, np.float32)


def main():
    torch.set_num_threads(8)
    out = {}
    for tag, seed, (B, g, S), per_image in (("a", SEED_A, (3, 5, 23), True), ("b", SEED_B, (2, 24, 336), False)):
        f, T, mask = SR.inputs(seed, B, g, S, per_image=per_image)
        r32 = reference_run(f, T, mask, S, torch.float32)
        r64 = reference_run(f, T, mask, S, torch.float64)
        mid = float(np.mean((r64["probs"] > 0.05) & (r64["probs"] < 0.95)))
        print(f"case {tag}: loss32 {r32['loss']:.7f} loss64 {r64['loss']:.7f}  p in (0.05, 0.95): {mid:.2%}  "
              f"dT32 rel-L2 {SR.rel_l2(r32['dT'], r64['dT']):.2e}  df32 rel-L2 {SR.rel_l2(r32['df'], r64['df']):.2e}")
        assert mid > 0.5
        o = dict(shape=np.array([B, g, S]), seed=np.array(seed), T=T, mask=mask.astype(np.uint8), mid_share=np.array(mid),
                 sums64=sums64(r64["probs"], mask), dT32=r32["dT"], dT64=r64["dT"], dgrid64=r64["dgrid"],
                 df32_rel=np.array(SR.rel_l2(r32["df"], r64["df"])))
        for k in ("loss", "focal", "dice0", "dice1"):
            o[k + "32"], o[k + "64"] = r32[k], r64[k]
        if tag == "a":
            o.update(f=f, rows=np.array(ROWS_A), df64=r64["df"].reshape(B * g * g, 768)[ROWS_A], dprobs64=r64["dprobs"],
                     adam_losses=adam_losses(f, T, mask, S))
            print("adam losses", o["adam_losses"])
        else:
            flat = f.reshape(B * g * g, 768)
            o.update(rows=np.array(ROWS_B), f_rows=flat[ROWS_B], f_sum=np.array(flat.astype(np.float64).sum()),
                     df64=r64["df"].reshape(B * g * g, 768)[ROWS_B], pix_step=np.array(PIX_STEP),
                     dprobs64=r64["dprobs"].ravel()[::PIX_STEP])
        out.update({f"{tag}_{k}": v for k, v in o.items()})
    path = os.path.join(HERE, "golden_segloss.npz")
    np.savez_compressed(path, **out)
    print("golden_segloss.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
