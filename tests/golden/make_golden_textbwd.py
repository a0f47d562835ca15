"""Generate tests/golden/golden_textbwd.npz by running the REAL reference's adapted text path
with its text adapter trainable (build machine only; needs the reference checkout
make_golden.py names).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_textbwd.py

Case "bottle": make_golden.build_reference()'s full-size synthetic model, the reference's own
get_adapted_single_class_text_embedding(model, "MVTec", "bottle") (forward_utils.py:138-162 over
model/adapter.py:114-145; 6 + 10 sentences) with text_adapter requiring grad, on the CPU in fp32
and in fp64. Loss L = sum G * T + 0.1 (T[:, 0] . T[:, 1])^2 with the seeded G of
textbwd_ref.loss_weights(). Stored: G, T32, T64, the losses; per adapter weight the fp64
gradient at the rows textbwd_ref.ROWS, its Frobenius norm and the fp32-vs-fp64 rel-L2 (the
yardstick); and, to localise a failure, dL/dx after blocks 11, 6, 2 and 0 (the block's own
output, before the adapter blend) for sentence 0 of the normal state, tokens 0..EOT, in fp64.

Case "adam": three Adam steps (betas (0.5, 0.999) as train.py:263-267, lr 1e-3) of the literal
loop body train.py:62-72, :87-100 with segloss_ref.inputs(ADAM_SEED, B=3, g=5, S=23) as the one
level's patch features and mask, class_names = [bottle, bottle, cable], text_norm_weight 0.1
(train.py:211). Four losses (three steps + the loss after the last step) in fp32, asserted here
to fall, and the same run in fp64 (what the 8x rule measures an fp32 run against).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from make_golden import HERE, REPO, build_reference  # noqa: E402 (sets sys.path: stubs, the reference, the repository)

sys.path.insert(0, os.path.join(REPO, "tests"))
import forward_utils as fu  # noqa: E402 (the reference's)
import segloss_ref as SR  # noqa: E402
import textbwd_ref as TR  # noqa: E402


def trainable_model(dtype):
    clip, model, sd, _, txt_ad = build_reference()
    model = model.to(dtype)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.text_adapter.parameters():
        p.requires_grad_(True)
    return clip, model, sd, txt_ad


def bottle_run(dtype, G):
    clip, model, sd, txt_ad = trainable_model(dtype)
    taps, hooks = {}, []
    for i in TR.TAPS:
        def mk(i):
            def hook(mod, inp, out):
                if i not in taps:  # the first encode_text call is the normal state
                    if out[0].requires_grad:
                        out[0].retain_grad()
                    else:  # block 0: nothing trainable below it, its output becomes a leaf
                        out[0].requires_grad_()
                    taps[i] = out[0]  # LND
            return hook
        hooks.append(model.clipmodel.transformer.resblocks[i].register_forward_hook(mk(i)))
    T = fu.get_adapted_single_class_text_embedding(model, "MVTec", "bottle", "cpu")
    for h in hooks:
        h.remove()
    loss = TR.fixture_loss(T, torch.from_numpy(G).to(dtype))
    loss.backward()
    grads = [model.text_adapter[i].fc[0].weight.grad.numpy() for i in range(4)]
    return dict(T=T.detach().numpy(), loss=float(loss.detach()), grads=grads,
                taps={i: t.grad[:, 0].numpy() for i, t in taps.items()}, sd=sd, txt_ad=txt_ad)


def adam_run(dtype):
    _, model, _, _ = trainable_model(dtype)
    f, _, mask = SR.inputs(TR.ADAM_SEED, 3, 5, 23)
    f, mask = torch.from_numpy(f).to(dtype), torch.from_numpy(mask).to(dtype)
    class_names = TR.ADAM_CLASSES
    opt = torch.optim.Adam(model.text_adapter.parameters(), lr=1e-3, betas=(0.5, 0.999))

    def step_loss():  # train.py:62-72, :87-96
        epoch_text_feature_dict = {}
        for class_name in list(set(class_names)):
            epoch_text_feature_dict[class_name] = fu.get_adapted_single_class_text_embedding(
                model, "MVTec", class_name, "cpu")
        epoch_text_feature = torch.stack([epoch_text_feature_dict[c] for c in class_names], dim=0)
        patch_preds = fu.calculate_similarity_map(f, epoch_text_feature, 23)
        loss = fu.calculate_seg_loss(patch_preds, mask)
        orthogonal_loss = ((epoch_text_feature[:, :, 0] * epoch_text_feature[:, :, 1]).sum(1).mean()) ** 2
        loss += orthogonal_loss * 0.1
        return loss

    losses = []
    for _ in range(3):
        loss = step_loss()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(step_loss()))
    return np.array(losses, np.float64)


def main():
    torch.set_num_threads(8)
    from model.tokenizer import tokenize
    from make_golden import class_sentences
    from dataset.constants import REAL_NAMES
    G = TR.loss_weights()
    r32, r64 = bottle_run(torch.float32, G), bottle_run(torch.float64, G)
    normal_s, abnormal_s = class_sentences(REAL_NAMES["MVTec"]["bottle"])
    tn, ta = tokenize(normal_s).numpy(), tokenize(abnormal_s).numpy()
    n_eot = int(tn[0].argmax()) + 1
    out = dict(G=G, T32=r32["T"], T64=r64["T"], loss32=np.array(r32["loss"]), loss64=np.array(r64["loss"]),
               rows=np.array(TR.ROWS), taps=np.array(TR.TAPS), n_eot=np.array(n_eot), tok_normal=tn, tok_abnormal=ta)
    print(f"bottle: {tn.shape[0]} + {ta.shape[0]} sentences, loss32 {r32['loss']:.7f} loss64 {r64['loss']:.7f}, "
          f"T32 rel-L2 {TR.rel_l2(r32['T'], r64['T']):.2e}")
    for i, (g32, g64) in enumerate(zip(r32["grads"], r64["grads"])):
        out[f"g{i}_rows64"] = g64[TR.ROWS]
        out[f"g{i}_norm64"] = np.array(np.linalg.norm(g64))
        out[f"g{i}_rel32"] = np.array(TR.rel_l2(g32, g64))
        print(f"  dW{i}: |g| {np.linalg.norm(g64):.4e}  fp32 rel-L2 {TR.rel_l2(g32, g64):.2e}")
        assert np.linalg.norm(g64) > 0
    for i in TR.TAPS:
        out[f"tap{i}_64"] = r64["taps"][i][:n_eot]
        tail = r64["taps"][i][n_eot:]
        print(f"  tap {i}: |dL/dx| {np.linalg.norm(out[f'tap{i}_64']):.4e}  fp32 rel-L2 "
              f"{TR.rel_l2(r32['taps'][i][:n_eot], out[f'tap{i}_64']):.2e}  after the EOT: max |.| {np.abs(tail).max():.1e}")
        out[f"tap{i}_rel32"] = np.array(TR.rel_l2(r32["taps"][i][:n_eot], out[f"tap{i}_64"]))
        assert np.abs(tail).max() == 0.0  # causal tower: no gradient behind an EOT (truncation is exact)
    # the restatement reproduces the reference (also pinned by tests/test_textbwd_host.py)
    rs = TR.run(r64["sd"], r64["txt_ad"], tn, ta, G, torch.float64)
    print("  restatement vs reference fp64: T", TR.rel_l2(rs["T"], r64["T"]),
          "grads", [TR.rel_l2(a, b) for a, b in zip(rs["grads"], r64["grads"])])
    a32, a64 = adam_run(torch.float32), adam_run(torch.float64)
    print("adam losses fp32", a32, "fp64", a64)
    assert all(b < a for a, b in zip(a32, a32[1:])), a32  # the reference's loss falls at each step
    out.update(adam_losses32=a32.astype(np.float32), adam_losses64=a64, adam_seed=np.array(TR.ADAM_SEED))
    path = os.path.join(HERE, "golden_textbwd.npz")
    np.savez_compressed(path, **out)
    print("golden_textbwd.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
