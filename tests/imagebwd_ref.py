"""Independent torch restatement of the adapted visual path (reference model/adapter.py:67-112),
written from the formulas and differentiable by autograd on the CPU. It runs in whatever dtype it
is asked for: fp64 is the truth the GPU tests compare with, fp32 on the CPU is the yardstick (the
error the reference's own arithmetic has). tests/test_imagebwd_host.py pins it to the real
reference's golden_imagebwd.npz.

  forward(P, ws, x)          [B, 3, S, S] -> (one [B, P, 768] per level, det [B, 768]): patch
                             embedding, ln_pre, 24 pre-LN blocks, the layer adapters after blocks
                             i < adapt_until, ln_post on the level taps, seg_proj / det_proj,
                             F.normalize, the patch mean of det
  run(sd, ad, x, G, dt)      L = sum_j sum(G_j * seg_j) + sum(G_d * det), backward: the outputs, the
                             11 weight gradients, dL/dx after the tapped blocks for image 0
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

LEVELS = (6, 12, 18, 24)
TAPS = (23, 18, 12, 6, 5, 0)      # blocks whose output gradient the fixture stores (image 0)
ROWS = list(range(5, 768, 48))    # the 16 rows of each weight gradient the fixture stores in fp64
COL_STEP = 4                      # ... at every 4th column
TAP_TOKENS = (0, 1, 32, 64)       # the tokens of image 0 whose dL/dx the fixture stores (CLS, first, middle, last)
IMG, BATCH = 112, 2               # 8 x 8 patches, 65 tokens: one full key tile and a tail of 1
G_SEED, X_SEED, ADAM_SEED = 911, 913, 912
ADAM_LR, ADAM_BETAS, ADAM_MILESTONES = 5e-4, (0.5, 0.999), (16000, 32000)
ADAM_ANCHORS = ("bottle_T_adapted", "brain_T_adapted")  # golden_text.npz: the per-image anchors [768, 2]
PATCH, WIDTH, EMBED = 14, 1024, 768


def rel_l2(a, b) -> float:
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def weight_names(adapt_until=6, n_levels=4, relu=False):
    """image_adapter state-dict keys in the order forward() takes the weights."""
    fc = ".fc.0.weight" if relu else ".fc.weight"
    return ([f"layer_adapters.{i}.fc.0.weight" for i in range(adapt_until)]
            + [f"seg_proj.{j}{fc}" for j in range(n_levels)] + ["det_proj" + fc])


def loss_weights(n_patch, seed=G_SEED, batch=BATCH, n_levels=4):
    """The seeded G of the fixture's loss: one [B, P, 768] per level and [B, 768] for det."""
    rng = np.random.default_rng(seed)
    return ([rng.standard_normal((batch, n_patch, EMBED)).astype(np.float32) for _ in range(n_levels)]
            + [rng.standard_normal((batch, EMBED)).astype(np.float32)])


def adam_inputs(img=IMG, batch=BATCH, seed=ADAM_SEED):
    """The seeded 0/1 mask [B, 1, S, S] and the labels [0, 1] of the three Adam steps."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((batch, 1, img, img), np.float32)
    for b in range(batch):
        y, x = (int(v) for v in rng.integers(0, img // 2, 2))
        mask[b, 0, y:y + img // 3, x:x + img // 2] = 1.0
    return mask, np.arange(batch, dtype=np.int64) % 2


def params(sd: dict, dtype) -> dict:
    """The visual tower's tensors out of a CLIP state dict (numpy or torch), in dtype."""
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if k.startswith("visual.")}


def _act(x, quick):
    return x * torch.sigmoid(1.702 * x) if quick else F.gelu(x)


def block(P, i, x, quick=False):
    """One pre-LN residual block on x [B, N, W], full attention."""
    p = f"visual.transformer.resblocks.{i}."
    B, N, W = x.shape
    H = W // 64
    h = F.layer_norm(x, (W,), P[p + "ln_1.weight"], P[p + "ln_1.bias"], 1e-5)
    qkv = h @ P[p + "attn.in_proj_weight"].T + P[p + "attn.in_proj_bias"]
    q, k, v = (t.reshape(B, N, H, 64).transpose(1, 2) for t in qkv.split(W, dim=-1))
    a = torch.softmax((q @ k.transpose(-1, -2)) / 8.0, dim=-1) @ v
    a = a.transpose(1, 2).reshape(B, N, W)
    x = x + a @ P[p + "attn.out_proj.weight"].T + P[p + "attn.out_proj.bias"]
    h = F.layer_norm(x, (W,), P[p + "ln_2.weight"], P[p + "ln_2.bias"], 1e-5)
    f = _act(h @ P[p + "mlp.c_fc.weight"].T + P[p + "mlp.c_fc.bias"], quick)
    return x + f @ P[p + "mlp.c_proj.weight"].T + P[p + "mlp.c_proj.bias"]


KINK_WINDOW = 1e-5  # |z| <= KINK_WINDOW * rms(z row): within an fp32 forward's error of LeakyReLU's kink


def _adapter_act(z, side, counter):
    """LeakyReLU(z). Its derivative jumps from 0.01 to 1 at z = 0, and among the ~800 k adapter
    pre-activations of the fixture the closest to 0 lie about 1e-6 rms away: an fp32 forward puts
    a few of them on the other side than fp64 does, and either slope is then a correct fp32
    answer (fp32 torch on the CPU itself moves 1e-4 .. 1e-3 in rel-L2 of a weight gradient with
    the thread count for that reason). side (optional, bool, z's shape): the side the run under
    test took; it decides the branch for the elements inside KINK_WINDOW, and only for those."""
    pos = z > 0
    if side is not None:
        near = z.detach().abs() <= KINK_WINDOW * z.detach().square().mean(-1, keepdim=True).sqrt()
        counter.append(int((near & (pos != side)).sum()))
        pos = torch.where(near, side, pos)
    return torch.where(pos, z, 0.01 * z)


def forward(P, ws, x, *, levels=LEVELS, adapt_until=6, i_w=0.1, relu=False, quick=False, taps=None, sides=None,
            moved=None):
    """x [B, 3, S, S] -> ([seg_j [B, P, 768]], det [B, 768]). ws: adapt_until layer-adapter weights,
    one seg_proj weight per level, the det_proj weight. taps: a dict {block: None} filled with the
    block outputs (pre-blend, grads retained). sides: {block: bool [B, N, W]}, see _adapter_act;
    moved: a list that receives, per adapted block, how many elements changed branch."""
    B, C, S, _ = x.shape
    g = S // PATCH
    cols = x.reshape(B, C, g, PATCH, g, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, C * PATCH * PATCH)
    t = cols @ P["visual.conv1.weight"].reshape(WIDTH, -1).T
    t = torch.cat([P["visual.class_embedding"].expand(B, 1, -1), t], 1) + P["visual.positional_embedding"]
    t = F.layer_norm(t, (WIDTH,), P["visual.ln_pre.weight"], P["visual.ln_pre.bias"], 1e-5)
    tokens = []
    for i in range(max(levels)):
        t = block(P, i, t, quick)
        if taps is not None and i in taps:
            if t.requires_grad:
                t.retain_grad()
            else:  # nothing trainable below (block 0): make the output a leaf so it collects a gradient
                t.requires_grad_()
            taps[i] = t
        if i < adapt_until:
            if sides is None:
                u = F.leaky_relu(t @ ws[i].T, 0.01)
            else:
                u = _adapter_act(t @ ws[i].T, sides[i], moved if moved is not None else [])
            u = u * t.norm(dim=-1, keepdim=True) / u.norm(dim=-1, keepdim=True)
            t = i_w * u + (1 - i_w) * t
        if i + 1 in levels:
            tokens.append(t[:, 1:])
    tokens = [F.layer_norm(v, (WIDTH,), P["visual.ln_post.weight"], P["visual.ln_post.bias"], 1e-5) for v in tokens]
    proj = lambda v, w: F.leaky_relu(v @ w.T, 0.01) if relu else v @ w.T  # noqa: E731
    L = len(levels)
    seg = [F.normalize(proj(v, ws[adapt_until + j]), dim=-1) for j, v in enumerate(tokens)]
    det = F.normalize(proj(tokens[-1], ws[adapt_until + L]), dim=-1).mean(1)
    return seg, det


def fixture_loss(seg, det, G):
    return sum((g * s).sum() for g, s in zip(G[:-1], seg)) + (G[-1] * det).sum()


def run(sd, adapter, x, G, dtype=torch.float64, *, adapt_until=6, levels=LEVELS, relu=False, quick=False, P=None,
        trainable=None, sides=None):
    """The forward, the fixture loss and its backward in `dtype` on the CPU. trainable: indices of the
    weights that require grad (None: all). sides: see _adapter_act. Returns numpy: seg, det, loss,
    grads (None where frozen), taps {block: dL/dx [n_tok, 1024] of image 0} and moved (elements per
    adapted block that took the other LeakyReLU branch because of sides)."""
    P = params(sd, dtype) if P is None else P
    names = weight_names(adapt_until, len(levels), relu)
    ws = [torch.as_tensor(np.asarray(adapter[n])).to(dtype) for n in names]
    for i, w in enumerate(ws):
        if trainable is None or i in trainable:
            w.requires_grad_()
    taps = {i: None for i in TAPS if i < max(levels)}
    moved = []
    seg, det = forward(P, ws, torch.as_tensor(np.asarray(x)).to(dtype), levels=levels, adapt_until=adapt_until,
                       relu=relu, quick=quick, taps=taps, sides=sides, moved=moved)
    loss = fixture_loss(seg, det, [torch.as_tensor(g).to(dtype) for g in G])
    loss.backward()
    tap_g = {i: (t.grad[0].numpy() if t.grad is not None else np.zeros(tuple(t.shape[1:]))) for i, t in taps.items()}
    return dict(seg=[s.detach().numpy() for s in seg], det=det.detach().numpy(), loss=float(loss.detach()),
                grads=[w.grad.numpy() if w.grad is not None else None for w in ws], taps=tap_g, moved=moved)
