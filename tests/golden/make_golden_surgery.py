"""Generate tests/golden/golden_surgery.npz by running the REAL reference's frozen image
paths (build machine only; needs the reference checkout make_golden.py names).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_surgery.py

Reference code on synthetic weights (oracle/synth.py, seed 111), images
synth.images(111, 3, 336):
  * the surgery tower: create_model + visual.DAPM_replace(DPAM_layer=20), then
    encode_image(x, [6, 12, 18, 24]) (train.py:235-243, :75) for the batch of 3, for x[:1]
    and for x[[0, 2]] (the reference's v-v attention mixes the images of a batch, so the
    three differ);
  * the plain tower: encode_image(x, []) and (x, [6, 12, 18, 24]);
  * AdaptedCLIP.forward_original(x) (model/adapter.py:55-63);
  * the stage-1 teacher feature of train.py:74-85 at level 24.
Token tensors are stored at the rows ROWS only (data, < 1 MB); every token's L2 norm is
stored for all rows. Patch-indexed outputs (forward_original, teacher) are stored at the
patch rows ROWS[1:] - 1 (row 0 is the CLS token, which they do not contain).
Yardsticks, per level, over the stored rows: rel_drop_one = image 0 in the batch x[[0, 2]]
against image 0 in the batch of 3; rel_plain = the plain tower against the surgery tower.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from make_golden import HERE, SEED, build_reference, synth, t  # noqa: E402 (sets sys.path)

ROWS = [0, 1, 24, 25, 288, 300, 575, 576]
LEVELS = [6, 12, 18, 24]
DPAM_LAYER = 20


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


@torch.no_grad()
def main():
    clip_surgery, _, sd, _, _ = build_reference()
    clip_surgery.visual.DAPM_replace(DPAM_layer=DPAM_LAYER)
    replaced = [i for i, r in enumerate(clip_surgery.visual.transformer.resblocks)
                if type(r.attn).__name__ == "Attention"]
    clip, adapted, _, _, _ = build_reference()
    x = t(synth.images(SEED, 3, 336))
    prow = [r - 1 for r in ROWS[1:]]

    pooled3, tok3 = clip_surgery.encode_image(x, LEVELS)
    pooled1, tok1 = clip_surgery.encode_image(x[:1], LEVELS)
    _, tok02 = clip_surgery.encode_image(x[[0, 2]], LEVELS)
    plain_pooled, none = clip.encode_image(x, [])
    assert none == []
    _, plain_tok = clip.encode_image(x, LEVELS)
    fo_patch, fo_cls = adapted.forward_original(x)

    # train.py:74-85, as written there
    image, adapted_model = x, adapted
    _, patch_features = clip_surgery.encode_image(image, [6, 12, 18, 24])
    cls_token, _ = adapted_model.clipmodel.encode_image(image, [])
    cls_token = cls_token / cls_token.norm(dim=-1, keepdim=True)
    patch_features = [
        clip_surgery.visual.ln_post(t[:, 1:, :]) for t in patch_features
    ]
    patch_features = [t @ clip_surgery.visual.proj for t in patch_features]
    patch_features = [
        t / t.norm(dim=-1, keepdim=True) for t in patch_features
    ]
    patch_features = [t + cls_token.unsqueeze(1) for t in patch_features]

    n = lambda a: a.numpy().astype(np.float32)  # noqa: E731
    tok3, tok1, tok02, plain_tok = ([n(a) for a in lv] for lv in (tok3, tok1, tok02, plain_tok))
    out = dict(
        rows=np.array(ROWS), patch_rows=np.array(prow), levels=np.array(LEVELS), dpam_layer=np.array(DPAM_LAYER),
        replaced_blocks=np.array(replaced), clip_sha=np.array(synth.state_checksum(sd)),
        image_sha=np.array(synth.state_checksum({"x": x.numpy()})),
        surg_tok3=np.stack([a[:, ROWS] for a in tok3]), surg_tok1=np.stack([a[:, ROWS] for a in tok1]),
        surg_norm3=np.stack([np.linalg.norm(a, axis=-1) for a in tok3]),
        surg_norm1=np.stack([np.linalg.norm(a, axis=-1) for a in tok1]),
        surg_pooled3=n(pooled3), surg_pooled1=n(pooled1),
        plain_pooled=n(plain_pooled), plain_tok24=plain_tok[-1][:, ROWS],
        fo_patch=n(fo_patch[0])[:, prow], fo_cls=n(fo_cls),
        teacher24=n(patch_features[-1])[:, prow],
        rel_drop_one=np.array([rel(a[0][ROWS], b[0][ROWS]) for a, b in zip(tok02, tok3)]),
        rel_plain=np.array([rel(a[:, ROWS], b[:, ROWS]) for a, b in zip(plain_tok, tok3)]),
        rel_drop_one_full=np.array([rel(a[0], b[0]) for a, b in zip(tok02, tok3)]),
        rel_plain_full=np.array([rel(a, b) for a, b in zip(plain_tok, tok3)]),
        rel_batch1_full=np.array([rel(a[0], b[0]) for a, b in zip(tok1, tok3)]),
    )
    path = os.path.join(HERE, "golden_surgery.npz")
    np.savez_compressed(path, **out)
    for k in ("replaced_blocks", "rel_drop_one", "rel_plain", "rel_drop_one_full", "rel_plain_full",
              "rel_batch1_full"):
        print(k, out[k])
    print("golden_surgery.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
