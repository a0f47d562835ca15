"""Generate tests/golden/golden_imagebwd.npz by running the REAL reference's adapted visual path
with its image adapter trainable (build machine only; needs the reference checkout make_golden.py
names).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_imagebwd.py

make_golden.build_reference(img_size=112): 8 x 8 patches, 65 tokens (one full key tile of the tiled
attention backward plus a tail of 1), B = 2 synthetic images, image_adapter trainable and everything
else frozen, on the CPU in fp32 and in fp64.

Case "grad": L = sum_j sum(G_j * seg_j) + sum(G_d * det) with the seeded G of
imagebwd_ref.loss_weights(). Stored: the losses, rows of the outputs; per image_adapter weight the
fp64 gradient at the rows imagebwd_ref.ROWS (every COL_STEP-th column: the file stays under 1 MiB),
its Frobenius norm and the fp32-vs-fp64 rel-L2 (the
yardstick); and, to localise a failure, dL/dx after blocks 23, 18, 12, 6, 5 and 0 (the block's own
output, before the adapter blend) for image 0 at the tokens imagebwd_ref.TAP_TOKENS in fp64, with the
fp32-vs-fp64 rel-L2 over all tokens.

Case "adam": three steps of the literal loop body train.py:134-159 (Adam betas (0.5, 0.999), lr
5e-4, MultiStepLR [16000, 32000] x 0.5 as train.py:268-274), labels [0, 1], the seeded mask of
imagebwd_ref.adam_inputs() and the per-image anchors bottle / brain of golden_text.npz. Four losses
(three steps + the loss after the last step) in fp32 and the same run in fp64. The reference's loss
rises at the first step (lr 5e-4 on the synthetic weights overshoots) and falls from there to below
its start; that is what is asserted here.

Case "relu": the "grad" losses and the seg_proj.1 gradient norm with relu=True.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from make_golden import HERE, REPO, build_reference  # noqa: E402 (sets sys.path: stubs, the reference, the repository)

sys.path.insert(0, os.path.join(REPO, "tests"))
import forward_utils as fu  # noqa: E402 (the reference's)
import imagebwd_ref as IR  # noqa: E402
from oracle import synth  # noqa: E402


def trainable_model(dtype, relu=False):
    _, model, sd, img_ad, _ = build_reference(relu=relu, img_size=IR.IMG)
    model = model.to(dtype)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.image_adapter.parameters():
        p.requires_grad_(True)
    return model, sd, img_ad


def grad_run(dtype, x, G, relu=False):
    model, sd, img_ad = trainable_model(dtype, relu)
    taps, hooks = {}, []
    for i in IR.TAPS:
        def mk(i):
            def hook(mod, inp, out):
                if out[0].requires_grad:
                    out[0].retain_grad()
                else:  # block 0: nothing trainable below it, its output becomes a leaf
                    out[0].requires_grad_()
                taps[i] = out[0]  # LND
            return hook
        hooks.append(model.image_encoder.transformer.resblocks[i].register_forward_hook(mk(i)))
    seg, det = model(torch.from_numpy(x).to(dtype))
    for h in hooks:
        h.remove()
    loss = IR.fixture_loss(seg, det, [torch.from_numpy(g).to(dtype) for g in G])
    loss.backward()
    sdk = dict(model.image_adapter.named_parameters())
    grads = [sdk[n].grad.numpy() for n in IR.weight_names(relu=relu)]
    return dict(seg=[s.detach().numpy() for s in seg], det=det.detach().numpy(), loss=float(loss.detach()),
                grads=grads, taps={i: t.grad[:, 0].numpy() for i, t in taps.items()}, sd=sd, img_ad=img_ad)


def adam_run(dtype, x, anchors):
    model, _, _ = trainable_model(dtype)
    mask_np, label_np = IR.adam_inputs()
    image, mask, label = torch.from_numpy(x).to(dtype), torch.from_numpy(mask_np).to(dtype), torch.from_numpy(label_np)
    epoch_text_feature = torch.from_numpy(anchors).to(dtype)
    img_size = IR.IMG
    optimizer = torch.optim.Adam(model.image_adapter.parameters(), lr=IR.ADAM_LR, betas=IR.ADAM_BETAS)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=list(IR.ADAM_MILESTONES), gamma=0.5)

    def step_loss():  # train.py:145-154
        patch_features, det_feature = model(image)
        loss = 0.0
        det_feature = det_feature.unsqueeze(1)
        cls_preds = torch.matmul(det_feature, epoch_text_feature)[:, 0]
        loss += F.cross_entropy(cls_preds, label)
        for f in patch_features:
            patch_preds = fu.calculate_similarity_map(f, epoch_text_feature, img_size)
            loss += fu.calculate_seg_loss(patch_preds, mask)
        return loss

    losses = []
    for _ in range(3):
        loss = step_loss()
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        losses.append(loss.item())
        scheduler.step()
    with torch.no_grad():
        losses.append(float(step_loss()))
    return np.array(losses, np.float64)


def main():
    torch.set_num_threads(8)
    x = synth.images(IR.X_SEED, IR.BATCH, IR.IMG)
    n_patch = (IR.IMG // IR.PATCH) ** 2
    G = IR.loss_weights(n_patch)
    r32, r64 = grad_run(torch.float32, x, G), grad_run(torch.float64, x, G)
    out = dict(rows=np.array(IR.ROWS), taps=np.array(IR.TAPS), loss32=np.array(r32["loss"]), loss64=np.array(r64["loss"]),
               seg_rows64=np.stack([s[:, ::21, ::IR.COL_STEP] for s in r64["seg"]]), det64=r64["det"],
               seg_rel32=np.array([IR.rel_l2(a, b) for a, b in zip(r32["seg"], r64["seg"])]))
    print(f"grad: loss32 {r32['loss']:.7f} loss64 {r64['loss']:.7f}, seg fp32 rel-L2 {out['seg_rel32']}")
    names = IR.weight_names()
    for i, (n, g32, g64) in enumerate(zip(names, r32["grads"], r64["grads"])):
        out[f"g{i}_rows64"] = g64[IR.ROWS][:, ::IR.COL_STEP]
        out[f"g{i}_norm64"] = np.array(np.linalg.norm(g64))
        out[f"g{i}_rel32"] = np.array(IR.rel_l2(g32, g64))
        print(f"  d {n}: |g| {np.linalg.norm(g64):.4e}  fp32 rel-L2 {IR.rel_l2(g32, g64):.2e}")
        assert np.linalg.norm(g64) > 0
    for i in IR.TAPS:
        out[f"tap{i}_64"] = r64["taps"][i][list(IR.TAP_TOKENS)]
        out[f"tap{i}_rel32"] = np.array(IR.rel_l2(r32["taps"][i], r64["taps"][i]))
        print(f"  tap {i}: |dL/dx| {np.linalg.norm(r64['taps'][i]):.4e}  fp32 rel-L2 {float(out[f'tap{i}_rel32']):.2e}")
    # the restatement reproduces the reference (also pinned by tests/test_imagebwd_host.py)
    rs = IR.run(r64["sd"], r64["img_ad"], x, G, torch.float64)
    print("  restatement vs reference fp64: loss", abs(rs["loss"] - r64["loss"]),
          "grads", [IR.rel_l2(a, b) for a, b in zip(rs["grads"], r64["grads"])])
    q32, q64 = grad_run(torch.float32, x, G, relu=True), grad_run(torch.float64, x, G, relu=True)
    out.update(relu_loss32=np.array(q32["loss"]), relu_loss64=np.array(q64["loss"]),
               relu_g_norm64=np.array(np.linalg.norm(q64["grads"][7])),
               relu_g_rel32=np.array(IR.rel_l2(q32["grads"][7], q64["grads"][7])))
    print(f"relu: loss32 {q32['loss']:.7f} loss64 {q64['loss']:.7f} |d seg_proj.1| {float(out['relu_g_norm64']):.4e} "
          f"fp32 rel-L2 {float(out['relu_g_rel32']):.2e}")
    gt = np.load(os.path.join(HERE, "golden_text.npz"))
    anchors = np.stack([gt[k] for k in IR.ADAM_ANCHORS]).astype(np.float32)
    a32, a64 = adam_run(torch.float32, x, anchors), adam_run(torch.float64, x, anchors)
    print("adam losses fp32", a32, "fp64", a64)
    # Adam's first step moves every weight by lr = 5e-4 whatever its gradient; on the synthetic tower that
    # overshoots (the reference's own loss: 6.26 -> 7.96), whatever the mask seed and the anchors, and
    # the next steps recover. What the reference shows, and what is asserted: it falls from step 1 on
    # and ends below where it began.
    assert all(b < a for a, b in zip(a32[1:], a32[2:])) and a32[3] < a32[0], a32
    out.update(adam_losses32=a32.astype(np.float32), adam_losses64=a64)
    path = os.path.join(HERE, "golden_imagebwd.npz")
    np.savez_compressed(path, **out)
    print("golden_imagebwd.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
